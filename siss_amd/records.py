"""What the task loops and the metrics share when they write records: the JSON-lines appender, the "non-finite becomes null" rule and
the one-step-late writer of the training log.  No device library is needed to import this module."""
import json
import math


def finite_or_none(x):
    """float(x), or None when it is NaN / +-inf (json.dumps would write a token no JSON reader accepts)."""
    x = float(x)
    return x if math.isfinite(x) else None


def append_jsonl(path, rec):
    """Append `rec` to `path` as one JSON line; returns rec."""
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")
    return rec


class LaggedLog:
    """The training log written one step late: a step's scalars travel to the host behind its kernels and are read (and logged) once
    the NEXT step is queued, so the device never waits for the host between steps.  `record(handle, meta)` makes a step's record,
    `say(rec, meta)` its console line.  On the way out of the `with` the last COMPLETED step is written, also when the next one
    raised (a failure of that last write is swallowed: it must not mask what ended the loop), and the file is closed."""

    def __init__(self, path, record, say):
        self.file, self.record, self.say, self.pending = open(path, "a"), record, say, None

    def push(self, handle, meta):
        self.flush()
        self.pending = (handle, meta)

    def flush(self):
        if self.pending is not None:
            rec = self.record(*self.pending)
            self.file.write(json.dumps(rec) + "\n")
            self.file.flush()
            self.say(rec, self.pending[1])
            self.pending = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            self.flush()
        except Exception:
            pass
        self.file.close()
