"""Test helper: make the contents of a fresh allocation controllable.  Nothing here is shipped.

Every device buffer of the product is allocated in Python (``torch.empty``, ``torch.empty_like``, ``Tensor.new_empty``; ``_Launch.new`` and
``_new_cl`` go through ``torch.empty``) and is correct only if the kernels write every element that anything later reads.  In a fresh process
a new block is almost always zero, the one value that hides a violation.  ``with filled(pattern) as rec:`` replaces the three functions for
its duration: each replacement calls the original, fills the WHOLE storage of the tensor it got on the current stream and returns that same
tensor (no copy: address, strides and memory format, hence the alignment-dependent routes, stay as they were).

    pattern   floating dtypes (byte fill)                       uint8 / int8   int16 / int32 / int64 (value fill)   bool
    'zero'    0x00                                              0x00           0                                    False
    'nan'     0xFF (a NaN in fp16, bf16, fp32 and fp64)         0xFF           1                                    True
    'big'     0x7B (fp16 61280, fp32 1.3e36, fp64 6.5e286)      0x7B           2                                    True

The wide integer buffers get small values on purpose: some are counters or index tables, and a kernel that wrongly reads one before writing
it must still stay inside its buffers.  A bit comparison of the results under different patterns catches the dependence all the same.

``rec.sites`` is the set of (file, function) of the innermost caller frame inside the package directory (file relative to it) of every
allocation that was filled, looking through the package's two pass-through allocators (``WRAPPERS``: an ``L.new(...)`` belongs to the
function that wrote it, not to ``_Launch.new``) and through comprehensions; ``rec.count`` the number of allocations.  Not re-entrant
(nesting raises), and not to be active during a graph capture or inside ``route_probe.launched``."""
import contextlib
import os
import sys

import torch

PATTERNS = ('zero', 'nan', 'big')
BYTE = {'zero': 0x00, 'nan': 0xFF, 'big': 0x7B}
VALUE = {'zero': 0, 'nan': 1, 'big': 2}
PACKAGE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sh-gan_amd') + os.sep
# the package's own pass-through allocators: an allocation made through one belongs to the function that called it
WRAPPERS = {('kernels.py', 'new'), ('kernels_f16.py', '_new_cl')}
COMPREHENSIONS = ('<listcomp>', '<setcomp>', '<dictcomp>', '<genexpr>')       # (frames of their own before Python 3.12: the function around them)

_BYTE_INTS = (torch.uint8, torch.int8)
_active = [None]


class Recorder:
    def __init__(self, pattern):
        self.pattern = pattern
        self.sites = set()
        self.count = 0


def _caller_site(depth):
    """(file relative to the package, function) of the innermost frame inside the package, or None."""
    f = sys._getframe(depth)
    while f is not None:
        name = f.f_code.co_filename
        if name.startswith(PACKAGE_DIR):
            site = (name[len(PACKAGE_DIR):].replace(os.sep, '/'), f.f_code.co_name)
            if site not in WRAPPERS and f.f_code.co_name not in COMPREHENSIONS:
                return site
        f = f.f_back
    return None


def _fill(t, pattern, empty):
    """Fill the whole storage behind ``t`` (not only the elements its strides reach)."""
    st = t.untyped_storage()
    if st.nbytes() == 0:
        return
    dt = t.dtype
    if dt.is_floating_point or dt.is_complex or dt in _BYTE_INTS:
        empty(0, dtype=torch.uint8, device=t.device).set_(st).fill_(BYTE[pattern])
    elif dt == torch.bool:
        empty(0, dtype=torch.uint8, device=t.device).set_(st).fill_(min(VALUE[pattern], 1))
    else:
        empty(0, dtype=dt, device=t.device).set_(st).fill_(VALUE[pattern])


@contextlib.contextmanager
def filled(pattern):
    if pattern not in PATTERNS:
        raise ValueError(f'pattern must be one of {PATTERNS} (got {pattern!r})')
    if _active[0] is not None:
        raise RuntimeError(f"alloc_fill.filled is not re-entrant: '{_active[0].pattern}' is active")
    rec = Recorder(pattern)
    o_empty, o_like, o_new = torch.empty, torch.empty_like, torch.Tensor.new_empty
    own_new = 'new_empty' in vars(torch.Tensor)               # (inherited from the C base class: restored by deleting the override)

    def done(t):
        if isinstance(t, torch.Tensor) and not t.is_meta:
            _fill(t, pattern, o_empty)
            rec.count += 1
            site = _caller_site(3)
            if site is not None:
                rec.sites.add(site)
        return t

    def empty(*args, **kw):
        return done(o_empty(*args, **kw))

    def empty_like(*args, **kw):
        return done(o_like(*args, **kw))

    def new_empty(self, *args, **kw):
        return done(o_new(self, *args, **kw))

    _active[0] = rec
    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield rec
    finally:
        torch.empty, torch.empty_like = o_empty, o_like
        if own_new:
            torch.Tensor.new_empty = o_new
        else:
            del torch.Tensor.new_empty
        _active[0] = None
