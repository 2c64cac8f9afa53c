"""A guarded, exact workspace for tests: every scratch buffer is exactly as large as its sizer said, lies between two
guard bands, and starts out filled with a chosen byte.

Production hands scratch out through `_C.Workspace.bytes`, which grows a request by half plus 4096 bytes, so a sizer that
reports too little, or a caller that hands the sizer the wrong arguments, stays invisible.  Inside `exact_scratch` the
same calls get `outer[GUARD:GUARD + n]` of a `torch.full((GUARD + n + GUARD,), fill)` buffer:

* `intact(log)` says whether a kernel wrote before or behind its scratch (a short sizer, a carve that disagrees with
  it, or wrong sizer arguments),
* two runs with different fills that give different results show a read before write,
* `requests(log)` lists what was asked for, so a test can hold each request to the sizer's value.

Plain Python and torch: it works on any device (tests/test_scratch_guard_cpu.py tests it on the CPU).  Guards see writes
only.  A read past the end of a scratch lands in the guard and changes nothing there; only the comparison of the results
under different fills can show it."""
import contextlib

import torch

from gradslam_amd import _C

# a condition of the harness, not a measurement: a multiple of 256 (the unit of gs_align, so every carved offset keeps
# its alignment), 16 times the largest fixed pad a sizer adds (4096), and cheap to compare
GUARD = 65536


class GuardLog(list):
    """[(name, nbytes, outer)] plus the byte the buffers were filled with"""

    def __init__(self, fill):
        super().__init__()
        self.fill = int(fill)


def _guarded(device, nbytes, fill):
    n = max(int(nbytes), 1)         # a zero-length tensor has a null data_ptr(); the log keeps the requested size
    outer = torch.full((GUARD + n + GUARD,), fill, dtype=torch.uint8, device=device)
    return outer, outer[GUARD:GUARD + n]


def guarded_buffer(log, name, nbytes, device):
    """One guarded buffer outside any Workspace (for tests that hand a scratch pointer to the C ABI themselves)."""
    outer, inner = _guarded(device, nbytes, log.fill)
    log.append((name, int(nbytes), outer))
    return inner


@contextlib.contextmanager
def exact_scratch(monkeypatch, fill):
    """Yields the log [(name, nbytes, outer)].  Workspaces made inside are dropped on exit and the earlier ones come back,
    so no pointer of a guarded buffer outlives the context: create objects that keep pointers (StepPlan) inside it."""
    log = GuardLog(fill)
    saved = dict(_C.Workspace._instances)
    _C.Workspace._instances.clear()

    def bytes_(self, name, nbytes):
        buf = self._bufs.get(name)
        if buf is None or buf.numel() < nbytes:     # the production reuse rule (the stats exporters rely on it)
            outer, buf = _guarded(self.device, nbytes, fill)
            self._bufs[name] = buf
            log.append((name, int(nbytes), outer))
        return buf

    try:
        with monkeypatch.context() as m:
            m.setattr(_C.Workspace, "bytes", bytes_)
            yield log
    finally:
        _C.Workspace._instances.clear()
        _C.Workspace._instances.update(saved)


def requests(log):
    return [(name, nbytes) for name, nbytes, _ in log]


def intact(log):
    """(True, []) if every byte of both guards of every logged buffer still holds the fill; else (False, hits) with one
    (name, side, first, last) per touched guard.  Offsets of the "trailing" side count from the first byte behind the
    scratch (0 is the byte a sizer short by one loses); those of the "leading" side are negative and count back from the
    scratch's first byte (-1 is the byte just before it)."""
    hits = []
    for name, nbytes, outer in log:
        n = max(nbytes, 1)
        for side, band, base in (("leading", outer[:GUARD], -GUARD), ("trailing", outer[GUARD + n:], 0)):
            if bool((band == log.fill).all()):
                continue
            hit = torch.nonzero(band != log.fill).flatten()
            hits.append((name, side, base + int(hit[0]), base + int(hit[-1])))
    return (not hits), hits
