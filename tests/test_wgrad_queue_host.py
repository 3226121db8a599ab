"""siss_amd/wgrad.py on the host: the weight-gradient queue against a recording launcher and a list for a buffer pool.

What is pinned here is the bookkeeping that whole-network parity only sees as slightly wrong gradients at some shape: WHEN an
operand returns to the pool (after the launch that reads it, never before), what a write to a held buffer forces, where a full
queue goes, and who pairs with whom at the top resolution.  CPU tensors stand in for device operands (a job only takes their
addresses); operands are objects with `.buf`, column views objects with `.base`.
"""
import contextlib
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

from siss_amd import lib, ops
from siss_amd.wgrad import WgradQueue


class _Queue(WgradQueue):
    """The two stream operations replaced: launches inside the fork are recorded as side-stream launches, the wait as an event."""
    on_side = False

    @contextlib.contextmanager
    def _on_side(self):
        self.on_side = True
        try:
            yield
        finally:
            self.on_side = False

    def _wait_side(self):
        self.eng.log.append(("WAIT_SIDE", (), False))


class _Engine:
    """What the queue reads from its owner: the live switches, the parameter store's size, the device, and the pool's _put."""
    group_max, side_follow, wgrad_side, side_blocks, f32, wgrad_overwrite = 3, 1, True, 128, False, False
    device = torch.device("cpu")

    def __init__(self, status=()):
        self.ps = NS(total=4096)
        self.log, self.pool, self.status = [], [], dict(status)
        self.wgrads = _Queue(self, launcher=self.launch)

    def launch(self, name, *args, refusable=False):
        self.log.append((name, args, self.wgrads.on_side))
        return self.status.get(name, 0)

    def _put(self, a):                                   # UNetEngine._put
        if a is not None and not self.wgrads.defer_release(a):
            self.pool.append(a)

    def names(self):
        return [(n, side) for n, _, side in self.log]


def _act():
    return NS(buf=torch.zeros(4))


def _job(q, panels=1, **kw):
    y, x, dw = torch.zeros(8), torch.zeros(8), torch.zeros(8)
    return q.job(y, 8, x, 8, dw, 4, 4, list(range(panels)), [0] * panels, nsets=2, rows_per_set=10, row_begin=1, row_end=9,
                 x_set_rows=0, **kw)


def test_builder_fills_every_field_and_pads_the_tap_tables_to_nine():
    eng = _Engine()
    y, x, dw, b1, b2 = (torch.zeros(16) for _ in range(5))
    got = eng.wgrads.job(y, 12, x, 20, dw, 24, 40, [-3, 0, 5, 6], [0, 8, 16, 24], nsets=2, rows_per_set=100, row_begin=7, row_end=93,
                         x_set_rows=100, nsplits=3, dbias=b1, dbias2=b2.data_ptr(), set_stride=640, bias_set_stride=77)
    want = lib.TNJob(Y=y.data_ptr(), ldy=12, X=x.data_ptr(), ldx=20, dW=dw.data_ptr(), set_stride=640, N=24, C=40, npanels=4, nsets=2,
                     rows_per_set=100, row_begin=7, row_end=93, nsplits=3, x_set_rows=100,
                     zero_page=ops.zero_page(eng.device).data_ptr(), dbias=b1.data_ptr(), dbias2=b2.data_ptr(),
                     shifts=(lib.I * 9)(-3, 0, 5, 6, 0, 0, 0, 0, 0), coffs=(lib.I * 9)(0, 8, 16, 24, 0, 0, 0, 0, 0), bias_set_stride=77)
    assert bytes(got) == bytes(want)
    for f, _ in lib.TNJob._fields_:                      # (field by field too: a failure then names the field)
        a, b = getattr(got, f), getattr(want, f)
        assert (list(a), f) == (list(b), f) if f in ("shifts", "coffs") else (a, f) == (b, f)
    # the defaults: one panel at shift 0, the flat gradient buffer's set stride, no bias gradients, the library's split choice
    d = eng.wgrads.job(y, 12, x, 20, dw, 24, 40, nsets=1, rows_per_set=5, row_begin=0, row_end=5, x_set_rows=0)
    assert (d.npanels, list(d.shifts), list(d.coffs)) == (1, [0] * 9, [0] * 9)
    assert (d.set_stride, d.bias_set_stride, d.dbias, d.dbias2, d.nsplits) == (4096, 0, None, None, 0)
    eng.wgrad_overwrite = True                           # ... read live: first micro-batch of a step, bf16
    assert _job(eng.wgrads).nsplits == -2 and _job(eng.wgrads, nsplits=0).nsplits == 0
    eng.f32 = True
    assert _job(eng.wgrads).nsplits == 0


def test_solo_launch_takes_its_own_split_count_and_the_first_npanels_taps():
    eng = _Engine()
    q = eng.wgrads
    j = _job(q, panels=4, nsplits=5)
    q.launch(j)
    q.launch(j, 7)
    (n0, a0, _), (n1, a1, _) = eng.log
    assert n0 == n1 == "siss_gemm_tn" and len(a0) == 20
    assert (a0[16], a1[16]) == (0, 7)                    # nsplits: the argument, never the job's 5
    assert (list(a0[9]), list(a0[10])) == ([0, 1, 2, 3], [0] * 4)
    assert a0[:9] == (j.Y, 8, j.X, 8, j.dW, 4096, 4, 4, 4) and a0[11:16] == (2, 10, 0, 1, 9) and a0[17:] == (j.zero_page, None, None)
    eng.log.clear()
    q.launch(_job(q, panels=4, nsplits=0, bias_set_stride=99))   # a bias gradient with a set stride of its own: the _bs entry point
    assert eng.log[0][0] == "siss_gemm_tn_bs" and eng.log[0][1][-1] == 99 and len(eng.log[0][1]) == 21


def test_operand_released_while_queued_reaches_the_pool_after_the_flush():
    eng = _Engine()
    q = eng.wgrads
    before, dy, never = _act(), _act(), _act()
    eng._put(before)                                     # released before anything was queued
    assert eng.pool == [before]
    q.queue(_job(q), hold=dy)
    eng._put(never)                                      # never an operand
    eng._put(dy)
    assert eng.pool == [before, never] and q.is_held(dy.buf) and not q.is_held(never.buf) and not q.idle
    q.flush()
    assert eng.pool == [before, never, dy] and not q.is_held(dy.buf) and q.idle
    assert eng.names() == [("siss_gemm_tn_grouped", False)]
    table, n = eng.log[0][1]
    assert n == 1 and len(table) == 1 and table._type_ is lib.TNJob
    eng._put(dy)                                         # the next release of the same buffer is immediate again
    assert eng.pool[-1] is dy and len(eng.pool) == 4


def test_operand_of_a_side_flush_reaches_the_pool_after_the_join():
    eng = _Engine()
    q = eng.wgrads
    side_dy, main_dy, unqueued = _act(), _act(), _act()
    q.queue(_job(q), hold=side_dy)
    q.queue(_job(q))                                     # operands in named buffers: no hold
    q.wait_for_partner(_job(q), main_dy)                 # held, but by no QUEUED job: stays with this stream
    eng._put(side_dy); eng._put(main_dy); eng._put(unqueued)
    assert eng.pool == [unqueued]
    q.flush_side()
    name, (table, n, cap), on_side = eng.log[0]
    assert (name, n, cap, on_side) == ("siss_gemm_tn_grouped_capped", 2, 128, True) and len(eng.log) == 1
    assert eng.pool == [unqueued] and q.is_held(side_dy.buf) and q.is_held(main_dy.buf)
    q.flush()                                            # a main flush does not release what the side stream still reads
    assert eng.pool == [unqueued, main_dy] and q.is_held(side_dy.buf) and not q.idle
    assert eng.names()[1:] == [("siss_gemm_tn", False)]  # (the leftover pair candidate)
    q.join()
    assert eng.pool == [unqueued, main_dy, side_dy] and eng.names()[2:] == [("WAIT_SIDE", False)] and q.idle
    q.join()                                             # nothing on the side stream: no wait
    assert len(eng.log) == 3


@pytest.mark.parametrize("off", [dict(wgrad_side=False), dict(side_blocks=7), dict(f32=True)])
def test_side_flush_falls_back_to_the_main_stream(off):
    eng = _Engine()
    q = eng.wgrads
    ran = []
    q.after_launch(lambda: ran.append(1))
    q.flush_side()                                       # empty job list: returns at once, hooks untouched
    assert eng.log == [] and ran == [] and not q.idle
    for k, v in off.items():
        setattr(eng, k, v)
    dy = _act()
    q.queue(_job(q), hold=dy)
    eng._put(dy)
    q.flush_side()
    assert eng.names() == [("siss_gemm_tn_grouped", False)] and ran == [1] and eng.pool == [dy] and q.idle


def test_side_flush_caps_at_a_multiple_of_eight_blocks():
    eng = _Engine()
    eng.side_blocks = 77
    eng.wgrads.queue(_job(eng.wgrads))
    eng.wgrads.flush_side()
    assert eng.log[0][1][2] == 72


def test_a_write_to_a_held_buffer_runs_the_launch_that_reads_it_first():
    eng = _Engine()
    q = eng.wgrads
    held, side, free = _act(), _act(), _act()
    q.queue(_job(q), hold=side)
    q.flush_side()
    q.queue(_job(q), hold=held)
    eng.log.clear()
    q.before_write(None)
    q.before_write(free)
    q.before_write(NS(base=free))
    assert eng.log == []
    q.before_write(NS(base=held))                        # a column view resolves through its base's buffer
    assert eng.names() == [("siss_gemm_tn_grouped", False)] and q.is_held(side.buf)
    q.before_write(held)                                 # ... and is free afterwards
    assert len(eng.log) == 1
    q.before_write(NS(base=side))
    assert eng.names()[1:] == [("WAIT_SIDE", False)] and q.idle


def test_full_queue_flushes_at_group_max_and_follows_the_side_phase():
    eng = _Engine()
    q = eng.wgrads
    for _ in range(2):
        q.queue(_job(q))
        q.flush_if_full()
    assert eng.log == []                                 # 2 < group_max = 3
    q.queue(_job(q))
    q.flush_if_full()
    assert eng.names() == [("siss_gemm_tn_grouped", False)] and eng.log[0][1][1] == 3
    eng.group_max = 1                                    # lowered on the owner after construction: read live
    q.queue(_job(q))
    q.flush_if_full()
    assert eng.names()[1:] == [("siss_gemm_tn_grouped", False)]
    q.queue(_job(q))
    q.begin_side_phase()                                 # what is queued goes to the side stream ...
    q.queue(_job(q))
    q.flush_if_full()                                    # ... and so does a queue that fills up later (side_follow)
    assert eng.names()[2:] == [("siss_gemm_tn_grouped_capped", True)] * 2
    eng.side_follow = 0
    q.queue(_job(q))
    q.flush_if_full()
    assert eng.names()[4:] == [("siss_gemm_tn_grouped", False)]
    eng.side_follow = 1
    q.end_side_phase()
    q.queue(_job(q))
    q.flush_if_full()
    assert eng.names()[5:] == [("siss_gemm_tn_grouped", False)]
    eng.group_max = 3
    for _ in range(5):                                   # a site that never asks: the queue may exceed group_max
        q.queue(_job(q))
    assert len(eng.log) == 6 and len(q.jobs) == 5
    q.drain()
    assert eng.names()[6:] == [("siss_gemm_tn_grouped", False), ("WAIT_SIDE", False)] and eng.log[6][1][1] == 5 and q.idle


def _addr(ref):
    """The job behind a byref() argument."""
    return ctypes.addressof(ref._obj)


def test_pairing_prefers_the_same_cotangent_and_releases_it_with_its_last_product():
    eng = _Engine()
    q = eng.wgrads
    assert q.pair(_job(q, panels=9), _act()) is False and eng.log == []      # nobody waits: the caller launches on its own
    old, dy = _act(), _act()
    j_old, j_a, j_b = _job(q), _job(q), _job(q)
    q.wait_for_partner(j_old, old)
    q.wait_for_partner(j_a, dy)
    q.wait_for_partner(j_b, dy)
    eng._put(dy); eng._put(old)
    assert eng.pool == []
    j3 = _job(q, panels=9)
    assert q.pair(j3, dy) is True
    name, (r3, r1, zero), _ = eng.log[0]
    assert name == "siss_gemm_tn_pair" and zero == 0 and (_addr(r3), _addr(r1)) == (ctypes.addressof(j3), ctypes.addressof(j_a))
    assert eng.pool == [] and q.is_held(dy.buf)          # j_b still reads dy
    assert q.pair(_job(q, panels=9), dy) is True
    assert _addr(eng.log[1][1][1]) == ctypes.addressof(j_b)
    assert eng.pool == [dy] and not q.is_held(dy.buf) and q.is_held(old.buf)
    assert q.pair(_job(q, panels=9), dy) is True         # no product over dy waits any more: the oldest
    assert _addr(eng.log[2][1][1]) == ctypes.addressof(j_old) and eng.pool == [dy, old] and q.idle


def test_refused_pair_runs_both_products_alone_with_split_count_zero():
    eng = _Engine(status={"siss_gemm_tn_pair": 1})
    q = eng.wgrads
    eng.wgrad_overwrite = True                           # both jobs carry nsplits = -2
    dy = _act()
    j1, j3 = _job(q), _job(q, panels=9)
    q.wait_for_partner(j1, dy)
    eng._put(dy)
    assert q.pair(j3, dy) is True
    assert [n for n, _ in eng.names()] == ["siss_gemm_tn_pair", "siss_gemm_tn", "siss_gemm_tn"]
    (_, a3, _), (_, a1, _) = eng.log[1:]
    assert (a3[8], a3[16], a1[8], a1[16]) == (9, 0, 1, 0) and (j1.nsplits, j3.nsplits) == (-2, -2)
    assert eng.pool == [dy] and q.idle


def test_leftover_pair_candidate_runs_alone_at_the_next_main_flush():
    eng = _Engine()
    q = eng.wgrads
    eng.wgrad_overwrite = True
    dy = _act()
    q.wait_for_partner(_job(q), dy)
    eng._put(dy)
    q.flush_side()                                       # no queued job: nothing happens, the candidate keeps waiting
    assert eng.log == [] and eng.pool == []
    q.flush()
    assert eng.names() == [("siss_gemm_tn", False)] and eng.log[0][1][16] == 0 and eng.pool == [dy] and q.idle


def test_post_hooks_follow_the_grouped_launch_of_the_next_flush():
    eng = _Engine()
    q = eng.wgrads
    hook = lambda tag: (lambda: eng.log.append((tag, (), q.on_side)))
    q.queue(_job(q))
    q.after_launch(hook("fold-a"))
    q.flush()
    assert eng.names() == [("siss_gemm_tn_grouped", False), ("fold-a", False)]
    q.flush()                                            # hooks run once
    assert len(eng.log) == 2
    q.after_launch(hook("fold-b"))                       # a main flush with an empty job list still runs them
    q.flush()
    assert eng.names()[2:] == [("fold-b", False)]
    q.queue(_job(q))
    q.after_launch(hook("fold-c"))                       # on the side stream: behind the capped launch, on ITS stream
    q.flush_side()
    assert eng.names()[3:] == [("siss_gemm_tn_grouped_capped", True), ("fold-c", True)]


def test_reset_forgets_the_pass_but_not_the_side_stream():
    eng = _Engine()
    q = eng.wgrads
    a, b = _act(), _act()
    q.queue(_job(q), hold=a)
    q.flush_side()
    q.queue(_job(q), hold=b)
    q.wait_for_partner(_job(q), b)
    q.after_launch(lambda: None)
    q.reset()
    assert not (q.jobs or q.pair1 or q.post or q.held or q.held_release) and not q.is_held(b.buf)
    assert q.side_busy and q.is_held(a.buf) and not q.idle
    q.join()
    assert q.idle
