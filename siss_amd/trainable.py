"""Which parameters an unlearning run updates: `deletion.trainable` (a list of regular expressions over the diffusers parameter names),
`SISSStepper(trainable=...)` (names, or the parameters' requires_grad flags), and what the rest of the package needs to know of
the selection -- ONE table of stretches of the flat parameter buffer.

The table has the form siss_zero_ranges takes (16-byte granules: n starts, then the n + 1 prefix sums of the lengths) and drives
siss_grad_norms_scale_ranges / siss_recombine_clip_adamw_ranges (csrc/optimizer.hip); the same stretches tell the weight-gradient
queue which products nobody reads (siss_amd/wgrad.py) and the data-parallel exchange which pieces to sum (siss_amd/step.py).
Host code only: numpy-free, no GPU needed until `Subset.table(device)`.
"""
import bisect
import re

GRANULE = 4            # floats per 16-byte granule


def parse_patterns(value, key="deletion.trainable"):
    """`deletion.trainable`: None (absent / null: every parameter, today's run) or the list of compiled expressions.  Refused, with
    the offending entry: anything but a list of strings, an empty list, an expression that does not compile."""
    if value is None:
        return None
    if isinstance(value, (str, bytes)) or not isinstance(value, (list, tuple)):
        raise ValueError(f"{key}={value!r}: null or a LIST of regular expressions is needed (e.g. +{key}=[attn2])")
    if len(value) == 0:
        raise ValueError(f"{key}=[]: an empty list selects no parameter -- leave the key out (or null) for the full update")
    out = []
    for entry in value:
        if not isinstance(entry, str) or entry == "":
            raise ValueError(f"{key}: entry {entry!r} is not a regular expression (a non-empty string)")
        try:
            out.append(re.compile(entry))
        except re.error as e:
            raise ValueError(f"{key}: entry {entry!r} does not compile as a regular expression ({e})") from None
    return out


def select(names, patterns, key="deletion.trainable", announce=True):
    """The names (in the given order) that any expression `re.search`es.  An expression that matches nothing is refused by name.
    A selection of EVERY parameter returns None -- the full update -- after saying so (announce)."""
    if patterns is None:
        return None
    names = list(names)
    hit = set()
    for pat in patterns:
        mine = [n for n in names if pat.search(n)]
        if not mine:
            raise ValueError(f"{key}: entry {pat.pattern!r} matches no parameter of this UNet ({len(names)} tensors, e.g. {names[0]!r})")
        hit.update(mine)
    if len(hit) == len(names):
        if announce:
            print(f"[siss_amd] {key}={[p.pattern for p in patterns]!r} matches every parameter: running the full update")
        return None
    return [n for n in names if n in hit]


def merge_stretches(stretches, max_gap=0):
    """Sorted (start, end) stretches with those at most max_gap apart merged."""
    out = []
    for a, b in sorted(stretches):
        if out and a - out[-1][1] <= max_gap:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(s) for s in out]


class Subset:
    """The trainable stretches of a ParamStore's flat buffer.  Each trainable tensor contributes [off, off + roundup(numel, align))
    (the alignment padding is inside the full-buffer passes already: its gradients and parameters are zero and stay zero); adjacent
    stretches are merged."""

    def __init__(self, specs, names, total, align):
        names = list(names)
        unknown = [n for n in names if n not in specs]
        if unknown:
            raise KeyError(f"trainable: no parameter named {unknown[:3]} ({len(unknown)} unknown)")
        if not names:
            raise ValueError("trainable: an empty selection -- pass None for the full update")
        assert align % GRANULE == 0 and total % GRANULE == 0
        self.names = tuple(sorted(set(names), key=lambda n: specs[n].off))
        self.total = int(total)
        self.tensors = len(self.names)
        self.params = sum(int(specs[n].numel) for n in self.names)
        self.all_tensors = len(specs)
        self.stretches = tuple(merge_stretches((specs[n].off, specs[n].off + -(-specs[n].numel // align) * align) for n in self.names))
        assert all(0 <= a < b <= total for a, b in self.stretches)
        self._starts = [a for a, _ in self.stretches]
        self._tables = {}

    @property
    def floats(self):
        return sum(b - a for a, b in self.stretches)

    def signature(self):
        """Hashable: two selections with the same signature freeze the same floats."""
        return self.stretches

    def host_table(self):
        """(starts + prefix sums, n, total granules): siss_zero_ranges' table as a list of ints."""
        starts = [a // GRANULE for a, _ in self.stretches]
        pre = [0]
        for a, b in self.stretches:
            pre.append(pre[-1] + (b - a) // GRANULE)
        return starts + pre, len(starts), pre[-1]

    def table(self, device):
        """The device table (built once per device and kept: a captured step holds its address), n, total granules."""
        import torch
        tab, n, granules = self.host_table()
        key = str(device)
        if key not in self._tables:
            self._tables[key] = torch.tensor(tab, dtype=torch.int64, device=device)
        return self._tables[key], n, granules

    def is_frozen(self, off, n):
        """No float of [off, off + n) is trainable."""
        i = bisect.bisect_right(self._starts, off) - 1
        if i >= 0 and self.stretches[i][1] > off:
            return False
        return not (i + 1 < len(self.stretches) and self.stretches[i + 1][0] < off + n)

    def pieces(self, max_pieces=48):
        """The stretches merged across the smallest gaps until at most max_pieces remain (one grouped collective's pieces: a summed
        frozen gap costs bytes on the wire, a piece a slot of the group)."""
        gaps = sorted({b[0] - a[1] for a, b in zip(self.stretches, self.stretches[1:])})
        out = self.stretches
        for gap in [0] + gaps:
            out = merge_stretches(self.stretches, gap)
            if len(out) <= max_pieces:
                break
        return out


def from_flags(named_parameters):
    """The names whose parameter has requires_grad set (the diffusers idiom: unet.requires_grad_(False), then p.requires_grad_(True)
    for a few)."""
    return [n for n, p in named_parameters if p.requires_grad]
