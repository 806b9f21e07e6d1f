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
    from torch.profiler import ProfilerActivity, profile
    out, names = None, set()
    for _ in range(attempts):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            out = fn()
            torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}        # (host operator names come along; the patterns name kernels only)
        if all(any_hit(p, names) for p in expect):
            break
    return out, names
