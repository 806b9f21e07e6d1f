"""Test helper: which HIP kernels a call launched.  ``launched(fn)`` runs ``fn`` under ``torch.profiler`` with the CUDA (HIP) activity,
synchronizes and returns (result, set of kernel names); the names are the demangled device symbols, template arguments included, so a
pattern can pin one instantiation (``conv_wino4_kernel<2, 16>``) or a whole family (``conv_wino4_kernel``).  Nothing here is shipped."""
import re

import torch


def _norm(s):
    return re.sub(r'\s*([<>,:()])\s*', r'\1', s)          # (spacing inside template argument lists varies; 'void name' keeps its space)


def hit(pattern, name):
    """True when ``pattern`` names the kernel ``name``: spacing-insensitive, and the pattern starts at an identifier boundary
    (``bias_act_kernel`` does not match ``f16::bias_act_backward_f16_kernel``, ``conv_wino_kernel`` not ``conv_wgrad_wino_kernel``)."""
    p, n = _norm(pattern), _norm(name)
    start = 0
    while True:
        k = n.find(p, start)
        if k < 0:
            return False
        if k == 0 or not (n[k - 1].isalnum() or n[k - 1] == '_'):
            return True
        start = k + 1


def any_hit(pattern, names):
    return any(hit(pattern, n) for n in names)


def launched(fn, expect=(), attempts=3):
    """-> (fn(), kernel names).  The tracer occasionally drops the events of a short region: with ``expect`` given, the call is repeated
    (at most ``attempts`` times) until every expected pattern shows up; the names of the last attempt are returned either way."""
    out, counts = launch_counts(fn, expect=expect, attempts=attempts)
    return out, set(counts)


def launch_counts(fn, expect=(), attempts=3, want=None):
    """-> (fn(), {name: launches}), the ``count`` of the profiler's averages (host operator names come along; the patterns name kernels
    only), for paths that show as a second launch of the same kernel.  ``want``: {pattern: launches}; the call is repeated like ``launched``'s
    while an expected pattern is absent OR a wanted count is short (the tracer can drop one of two launches as well as both)."""
    from torch.profiler import ProfilerActivity, profile
    out, counts = None, {}
    for _ in range(attempts):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = fn()
            torch.cuda.synchronize()
        counts = {e.key: int(e.count) for e in prof.key_averages()}
        if all(any_hit(p, counts) for p in expect) and all(count_of(p, counts) >= n for p, n in (want or {}).items()):
            break
    return out, counts


def count_of(pattern, counts):
    return sum(n for name, n in counts.items() if hit(pattern, name))
