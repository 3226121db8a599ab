"""How a weight-gradient (TN) product gets launched, and how long its operands stay out of the buffer pool.

Nothing in a backward pass waits for a weight gradient (they only feed the flat gradient buffer), so an engine does not have to
launch one where its closure forms it.  :class:`WgradQueue` is the one owner of that freedom: a closure DESCRIBES its product once
(``job``) and says how it may run -- queued for a grouped launch (``queue``), waiting at the top resolution for a three-tap
partner (``wait_for_partner`` / ``pair``), or on its own (``launch``); the engine's schedule says WHEN the queue runs (``flush``,
``begin_side_phase``, ``join``, ``drain``); and the buffer pool asks before it overwrites or takes back an activation
(``before_write``, ``is_held``, ``defer_release``).  The measurements behind the switches it reads are with the switches, on
UNetEngine.
"""
import torch

from . import lib, ops


class WgradQueue:
    """The queued weight-gradient products of ONE engine.  The switches (group_max, side_follow, wgrad_side, side_blocks,
    wgrad_overwrite) are read from the engine at every decision: tests and bench.py flip them on an instance between passes.
    launcher: what runs a launch, (name, *args, refusable=False) -> status; default: lib.call, looked up at every launch."""

    def __init__(self, eng, launcher=None):
        self.eng, self.launcher = eng, launcher
        self.side_busy, self.side_held, self.side_release = False, {}, []
        self.side_phase = False
        self.frozen = None                               # siss_amd.trainable.Subset: the stretches of a gradient set somebody reads
        self.issued = self.dropped = 0                   # products described and kept / dropped since the engine was built
        self.reset()

    def reset(self):
        """Start of a forward pass: nothing queued, nothing waiting, nothing held (what the side stream still runs stays)."""
        self.jobs, self.held, self.held_release = [], {}, []      # jobs: (job, held cotangent operand or None)
        self.pair1 = []                                            # one-panel top-resolution products waiting: (job, cotangent)
        self.post = []                                             # hooks for the launch that forms the products queued so far

    @property
    def idle(self):
        return not (self.jobs or self.pair1 or self.post or self.held or self.side_busy)

    def _call(self, name, *args, **kw):
        return (self.launcher or lib.call)(name, *args, **kw)

    # ------------------------------------------------------------------ products nobody reads
    def set_frozen(self, subset):
        """subset (siss_amd.trainable.Subset, or None: every parameter is read): the optimizer reads the listed stretches of each
        gradient set and nothing else, so a product whose EVERY output lies outside them is dropped by job() -- while the engine's
        skip_frozen_wgrad is set."""
        self.frozen = subset

    def all_frozen(self, *outputs):
        """outputs: (tensor or address or None, floats per set, floats between sets, sets).  True when each is a window of the
        engine's gradient buffer that no listed stretch touches, in every set (an output anywhere else -- a scratch -- is read by
        somebody: False)."""
        fz, g = self.frozen, self.eng.ps.grads
        if fz is None or not getattr(self.eng, "skip_frozen_wgrad", True):
            return False
        base, total, nfloats = g.data_ptr(), g.shape[1], g.numel()
        for t, n, stride, sets in outputs:
            a = t.data_ptr() if torch.is_tensor(t) else t
            if not a:
                continue
            for s in range(sets):
                off, rem = divmod(a - base, 4)
                off += s * stride
                if rem or off < 0 or off + n > nfloats or off // total != (off + n - 1) // total or not fz.is_frozen(off % total, n):
                    return False
        return True

    # ------------------------------------------------------------------ describing a product
    def job(self, Y, ldy, X, ldx, dW, N, C, shifts=(0,), coffs=(0,), *, nsets, rows_per_set, row_begin, row_end, x_set_rows,
            nsplits=None, dbias=None, dbias2=None, set_stride=None, bias_set_stride=0):
        """dW[set] (+)= Y^T X over rows [row_begin, row_end) of every set, as a siss_tn_job.  Y, X, dW, dbias, dbias2: tensors or
        raw addresses.  nsplits None: the library chooses -- and overwrites instead of accumulating in the first micro-batch of
        a step (wgrad_overwrite).  set_stride None: dW is a window of the flat gradient buffer.  Returns None for a product that is
        DROPPED: dW, dbias and dbias2 all lie in frozen stretches of the gradient buffer (set_frozen) -- the caller neither queues,
        pairs nor launches it."""
        eng = self.eng
        addr = lambda t: t.data_ptr() if torch.is_tensor(t) else t
        pad9 = lambda v: (lib.I * 9)(*v, *([0] * (9 - len(v))))
        if nsplits is None:
            nsplits = -2 if (eng.wgrad_overwrite and not eng.f32) else 0
        zp = ops.zero_page(eng.device)
        j = lib.TNJob(Y=addr(Y), ldy=ldy, X=addr(X), ldx=ldx, dW=addr(dW),
                      set_stride=eng.ps.total if set_stride is None else set_stride, N=N, C=C, npanels=len(shifts), nsets=nsets,
                      rows_per_set=rows_per_set, row_begin=row_begin, row_end=row_end, nsplits=nsplits, x_set_rows=x_set_rows,
                      zero_page=zp.data_ptr(), dbias=addr(dbias), dbias2=addr(dbias2), shifts=pad9(shifts), coffs=pad9(coffs),
                      bias_set_stride=bias_set_stride)
        j.operands = (Y, X, dW, dbias, dbias2)            # (the job holds addresses: the tensors live as long as it does)
        if self.frozen is not None:
            bs = bias_set_stride or j.set_stride
            if self.all_frozen((j.dW, len(shifts) * N * C, j.set_stride, nsets), (j.dbias, N, bs, nsets), (j.dbias2, N, bs, nsets)):
                self.dropped += 1
                return None
        self.issued += 1
        return j

    # ------------------------------------------------------------------ running one
    def launch(self, job, nsplits=0):
        """On its own, now, on the current stream -- with THIS split count, whatever the job carries."""
        bs = job.bias_set_stride                          # (a bias gradient whose set stride is not dW's: the _bs entry point)
        self._call("siss_gemm_tn_bs" if bs else "siss_gemm_tn", job.Y, job.ldy, job.X, job.ldx, job.dW, job.set_stride, job.N, job.C,
                   job.npanels, lib.int_array(list(job.shifts)[:job.npanels]), lib.int_array(list(job.coffs)[:job.npanels]),
                   job.nsets, job.rows_per_set, job.x_set_rows, job.row_begin, job.row_end, nsplits, job.zero_page, job.dbias,
                   job.dbias2, *([bs] if bs else []))

    def queue(self, *jobs, hold=None):
        """For the next grouped launch.  hold: the Act these jobs read as their cotangent; it stays out of the pool until they ran
        (operands in per-site named buffers need none)."""
        self.jobs += [(j, hold) for j in jobs]
        if hold is not None:
            self.held[id(hold.buf)] = hold

    def after_launch(self, fn):
        """fn() right after the launch that forms the products queued so far, on its stream."""
        self.post.append(fn)

    def flush_if_full(self):
        """group_max products are a launch: beside the low-resolution middle of the pass on the side stream, else here."""
        if len(self.jobs) >= self.eng.group_max:
            self.flush_side() if (self.side_phase and self.eng.side_follow) else self.flush()

    # ------------------------------------------------------------------ top-resolution pairs
    def wait_for_partner(self, job, dy):
        """A one-panel product waits for the next three-tap product (or the next flush) and holds its cotangent dy."""
        self.pair1.append((job, dy))
        self.held[id(dy.buf)] = dy

    def pair(self, job, dy):
        """Offer the three-tap product `job` over dy to a waiting one-panel product: both run in one launch.  False: none waits."""
        if not self.pair1:
            return False
        # the partner: a waiting product over the SAME cotangent (the resnet's own conv_shortcut: its Y tiles are in L2), else the oldest
        same = [i for i, (_, d) in enumerate(self.pair1) if d is dy]
        j1, dy1 = self.pair1.pop(same[0] if same else 0)
        # (the launcher refuses a pair it cannot split over the device -- fewer CUs than the 3-tap product's base grid needs, no
        # room for a one-tap block: status 1 -- the two products then run as launches of their own)
        if self._call("siss_gemm_tn_pair", lib.C.byref(job), lib.C.byref(j1), 0, refusable=True):
            self.launch(job)
            self.launch(j1)
        if not any(d is dy1 for _, d in self.pair1):
            self._unhold(dy1)
        return True

    def _unhold(self, dy):
        """A waiting product that read `dy` has been launched: give the buffer back if its owner already released it."""
        self.held.pop(id(dy.buf), None)
        for a in [a for a in self.held_release if a.buf is dy.buf]:
            self.held_release.remove(a)
            self.eng._put(a)

    # ------------------------------------------------------------------ running the queue
    def _table(self):
        return (lib.TNJob * len(self.jobs))(*[j for j, _ in self.jobs]), len(self.jobs)

    def _run_post(self):
        post, self.post = self.post, []
        for fn in post:                                  # launches that consume a queued product (the sub-pixel upsample's tap fold)
            fn()

    def flush(self):
        """Run the queued products as grouped launches here and give every held operand back to the pool."""
        if self.jobs:
            self._call("siss_gemm_tn_grouped", *self._table())
            self.jobs = []
        self._run_post()
        for job, _ in self.pair1:                       # one-panel top-resolution products that found no 3-tap partner: on their own
            self.launch(job)
        self.pair1 = []
        self.held = {}
        rel, self.held_release = self.held_release, []
        for a in rel:
            self.eng._put(a)

    def _on_side(self):
        """Fork: the side stream, behind everything issued here so far, as the current stream of a `with` block."""
        side = self.eng._side_stream()
        side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(side)

    def _wait_side(self):
        torch.cuda.current_stream().wait_stream(self.eng._side_stream())

    def flush_side(self):
        """The queued products as CAPPED grouped launches on the side stream (behind everything issued so far)."""
        eng = self.eng
        if not self.jobs:
            return
        if not (eng.wgrad_side and eng.side_blocks >= 8) or eng.f32:
            return self.flush()
        with self._on_side():
            self._call("siss_gemm_tn_grouped_capped", *self._table(), int(eng.side_blocks) & ~7)
            self._run_post()
        for _, dy in self.jobs:                          # their cotangent operands stay out of the pool until the join
            if dy is not None and id(dy.buf) in self.held:
                self.side_held[id(dy.buf)] = self.held.pop(id(dy.buf))
        keep = []
        for a in self.held_release:
            (self.side_release if id(a.buf) in self.side_held else keep).append(a)
        self.held_release = keep
        self.jobs = []
        self.side_busy = True

    def join(self):
        """The launches on the side stream have to be complete before what follows on this stream; their operands return to the pool."""
        if not self.side_busy:
            return
        self._wait_side()
        self.side_busy, self.side_held = False, {}
        rel, self.side_release = self.side_release, []
        for a in rel:
            self.eng._put(a)

    def begin_side_phase(self):
        """The pass enters its low-resolution middle: what is queued so far runs beside it, and later full queues follow (side_follow)."""
        self.side_phase = True
        self.flush_side()

    def end_side_phase(self):
        self.side_phase = False

    def drain(self):
        """Everything queued, waiting or on the side stream is complete (in stream order) for what follows here."""
        self.flush()
        self.join()

    # ------------------------------------------------------------------ what the buffer pool asks
    def before_write(self, a):
        """`a` (Act, ActView or None) is about to be overwritten: a product that still reads its buffer must run first."""
        if a is None:
            return
        key = id(getattr(a, "base", a).buf)
        if key in self.held:
            self.flush()
        if key in self.side_held:
            self.join()

    def is_held(self, buf):
        return id(buf) in self.held or id(buf) in self.side_held

    def defer_release(self, a):
        """True: `a` is still read by a queued / side-stream product and goes back to the pool (eng._put) after the flush / join."""
        if self.held and id(a.buf) in self.held:
            self.held_release.append(a)
            return True
        if self.side_held and id(a.buf) in self.side_held:
            self.side_release.append(a)
            return True
        return False
