"""Test helper: house every fresh buffer between two poisoned guard bands and tell afterwards whether a band was touched.  Nothing here is
shipped.

The HIP library never allocates: every output, workspace and scratch buffer is made in Python and the kernels receive bare pointers.  A
kernel that stores one ragged tile, one float4, one pitch row or one split-K slice past the end of its buffer (or in front of it), or
that relies on a workspace formula that is a little short, damages nothing a test looks at: torch's caching allocator rounds every block
up to 512 bytes and the neighbour beyond that is usually a tensor nobody compares any more.  ``with guarded(band, operands) as rec:``
replaces, for its duration, the functions through which buffers come into being:

    FACTORIES   torch.empty / zeros / ones / full, their ``*_like`` forms, Tensor.new_empty / new_zeros / new_ones / new_full
    OPERANDS    Tensor.to / Tensor.cuda (``operands=True``), for the calls that turn a host tensor into a device tensor: the inputs and
                weights of a case are then housed the same way.  Every other ``.to`` (a cast, a host tensor staying on the host, a call
                autograd records) passes through.

Each replacement calls the original, reads size, strides, dtype, device, pinned-ness and ``requires_grad`` off its result, drops it and
returns a tensor with exactly those (memory format and ``is_contiguous`` answers included) whose storage is the interior of a larger raw
byte buffer: ``band`` bytes of guard, the tensor's storage bytes, ``band`` bytes of guard.  The trailing guard starts at the first byte
after the storage, not at a rounded address.  ``band`` is a multiple of 512, so the interior keeps the alignment modulo 512 bytes the
allocator gives any block, and no alignment-dependent route changes.  The interior is zero-filled (independence from its contents is the
subject of tests/alloc_fill.py, not of this helper); an initialising factory or a copy from the host then writes its own values.

    guard poison    floating, complex, uint8 / int8: byte 0xFF (a NaN in fp16, bf16, fp32 and fp64)      bool: True (byte 0x01)
                    int16 / int32 / int64: the value 3, written as elements

The wide integers get a small value for the reason alloc_fill gives them one: a kernel that wrongly reads an index or a counter from
the guard must still stay inside its buffers.  A guard value that reaches a result shows as a difference against an unguarded run.

``rec.violations()`` synchronises and compares every guard with its poison on the device.  It returns one ``Violation`` per damaged
band: site, factory, shape, dtype, the side ('front' / 'back'), the number of damaged bytes, the first and last damaged offset measured
from the tensor's boundary in bytes and in elements (back: 0 is the first byte after the storage; front: -1 is the last byte before it)
and the first few values found there -- enough to tell a ragged tile from a pitch row from a short workspace.

THE LIMIT OF WHAT THIS SEES.  A contiguous overrun begins at the boundary, so any band catches it.  A strided overrun lands within one
pitch row, one tile, one plane or one split-K slice of the end; the check sees it only if that unit is smaller than ``band``.  At the
shapes of the suite's case tables every such unit is below the default of 1 MiB.  An access further away than ``band`` leaves the memory
this helper owns and is not seen (and may fault).  A store of the poison value itself is not seen either, nor is a load whose value never
reaches a result.  Two bands per allocation cost 2 MiB each; the raw buffers live until the context ends so that no guarded block is
recycled inside a case (a few GB for the module-level cases).

``rec.sites`` is the set of (file, function) of ``alloc_fill._caller_site`` (``WRAPPERS`` looked through) over every allocation housed,
``rec.sites_of(factories)`` the same for some factories only, ``rec.count`` the number, ``rec.allocations`` the records.  Not re-entrant,
and ``guarded`` and ``alloc_fill.filled`` refuse to nest in each other (they share one slot).  Not to be active during a graph capture
(it raises) or inside ``route_probe.launched``.  Meta tensors, non-strided layouts, tensor subclasses and ``out=`` calls pass through."""
import contextlib

import numpy as np
import torch

import alloc_fill
from alloc_fill import _caller_site

EMPTY = ('empty', 'empty_like', 'new_empty')
INITIALISING = ('zeros', 'ones', 'full', 'zeros_like', 'ones_like', 'full_like', 'new_zeros', 'new_ones', 'new_full')
FACTORIES = EMPTY + INITIALISING
OPERANDS = ('to', 'cuda')
_FUNCTIONS = ('empty', 'empty_like', 'zeros', 'ones', 'full', 'zeros_like', 'ones_like', 'full_like')       # attributes of ``torch``
_METHODS = ('new_empty', 'new_zeros', 'new_ones', 'new_full')                                               # attributes of ``torch.Tensor``
BYTE_POISON = 0xFF
WIDE_POISON = 3
_BYTE_INTS = (torch.uint8, torch.int8)
FIRST_VALUES = 4


def poison_of(dtype):
    """('byte', value) or ('elem', value): how the guards of a buffer of this dtype are written and compared."""
    if dtype.is_floating_point or dtype.is_complex or dtype in _BYTE_INTS:
        return 'byte', BYTE_POISON
    if dtype == torch.bool:
        return 'byte', 1
    return 'elem', WIDE_POISON


def _itemsize(dtype):
    return torch.tensor([], dtype=dtype).element_size()            # (``torch.tensor`` is not one of the replaced factories)


class Allocation:
    def __init__(self, raw, nbytes, tensor, factory, site):
        self.raw, self.nbytes, self.factory, self.site = raw, nbytes, factory, site
        self.shape, self.dtype, self.device = tuple(tensor.shape), tensor.dtype, tensor.device


class Violation:
    def __init__(self, a, side, nbytes, first_byte, last_byte, values):
        self.site, self.factory, self.shape, self.dtype = a.site, a.factory, a.shape, a.dtype
        self.side, self.bytes, self.first_byte, self.last_byte, self.values = side, nbytes, first_byte, last_byte, values
        item = _itemsize(a.dtype)
        self.first_element, self.last_element = first_byte // item, last_byte // item

    def __repr__(self):
        return (f'<{self.site} {self.factory} {self.shape} {self.dtype}: side {self.side}, {self.bytes} bytes at offset {self.first_byte} .. '
                f'{self.last_byte} (elements {self.first_element} .. {self.last_element}), found {self.values}>')


class Recorder:
    pattern = 'guarded'               # (what ``alloc_fill.filled`` names when it refuses to nest)

    def __init__(self, band):
        self.band = band
        self.allocations = []
        self.sites = set()
        self.count = 0
        self.closed = False

    def sites_of(self, factories):
        return {a.site for a in self.allocations if a.factory in factories and a.site is not None}

    def _guards(self, a):
        kind, value = poison_of(a.dtype)
        front, back = a.raw[:self.band], a.raw[self.band + a.nbytes:]
        if kind == 'elem':
            front, back = front.view(a.dtype), back.view(a.dtype)
        return (('front', front), ('back', back)), value

    def violations(self):
        if self.closed:
            raise RuntimeError('alloc_guard: the guards are released when the context ends; call violations() inside it')
        if any(a.device.type == 'cuda' for a in self.allocations):
            torch.cuda.synchronize()
        flags = {}
        for k, a in enumerate(self.allocations):
            sides, value = self._guards(a)
            for side, g in sides:
                flags.setdefault(a.device, []).append(((k, side, g, value), (g != value).any()))
        found = []
        for dev, items in flags.items():
            hit = torch.stack([f for _, f in items]).cpu().tolist()
            for ((k, side, g, value), _), bad in zip(items, hit):
                if bad:
                    found.append(self._describe(self.allocations[k], side, g, value))
        return found

    def _describe(self, a, side, g, value):
        got = g.cpu().contiguous().numpy()
        want = np.full_like(got, value)
        bad = np.nonzero(got.view(np.uint8) != want.view(np.uint8))[0]
        first, last = int(bad[0]), int(bad[-1])
        size = _itemsize(a.dtype)
        lo = first // size * size
        chunk = got.view(np.uint8)[lo:lo + FIRST_VALUES * size].copy()
        try:
            values = torch.from_numpy(chunk).view(a.dtype).tolist()
        except (RuntimeError, TypeError):
            values = chunk.tolist()
        if side == 'front':
            first, last = first - self.band, last - self.band
        return Violation(a, side, int(bad.size), first, last, values)


@contextlib.contextmanager
def guarded(band=1 << 20, operands=True):
    if band <= 0 or band % 512:
        raise ValueError(f'band must be a positive multiple of 512 bytes (got {band})')
    if alloc_fill._active[0] is not None:
        raise RuntimeError(f"alloc_guard.guarded is not re-entrant and does not nest with alloc_fill.filled: '{alloc_fill._active[0].pattern}' is active")
    rec = Recorder(band)
    o_fn = {n: getattr(torch, n) for n in _FUNCTIONS}
    methods = _METHODS + (OPERANDS if operands else ())
    o_me = {n: getattr(torch.Tensor, n) for n in methods}
    own = {n: n in vars(torch.Tensor) for n in methods}                    # (inherited from the C base class: restored by deleting the override)
    o_empty = o_fn['empty']

    def house(r, factory, copy):
        """The guarded twin of ``r``, the result of the original call; ``r`` itself where the guard has nothing to house."""
        if type(r) is not torch.Tensor or r.is_meta or r.layout != torch.strided or r.device.type not in ('cpu', 'cuda') or r.storage_offset() != 0:
            return r
        if r.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('alloc_guard.guarded must not be active during a graph capture')
        nbytes, item = r.untyped_storage().nbytes(), r.element_size()
        if nbytes % item:
            return r
        kw = dict(pin_memory=True) if r.device.type == 'cpu' and r.is_pinned() else {}
        raw = o_empty(2 * band + nbytes, dtype=torch.uint8, device=r.device, **kw)
        kind, value = poison_of(r.dtype)
        if kind == 'byte':
            raw.fill_(value)
        else:
            raw[:band].view(r.dtype).fill_(value)
            raw[band + nbytes:].view(r.dtype).fill_(value)
        raw[band:band + nbytes].zero_()
        g = o_empty(0, dtype=r.dtype, device=r.device).set_(raw.untyped_storage(), band // item, r.size(), r.stride())
        if copy and nbytes:
            with torch.no_grad():
                g.copy_(r.detach())
        if r.requires_grad:
            g.requires_grad_(True)
        site = _caller_site(3)
        rec.allocations.append(Allocation(raw, nbytes, g, factory, site))
        rec.count += 1
        if site is not None:
            rec.sites.add(site)
        return g

    def function(name):
        orig, copy = o_fn[name], name in INITIALISING

        def replacement(*args, **kw):
            r = orig(*args, **kw)
            return r if kw.get('out') is not None else house(r, name, copy)
        replacement.__name__ = name
        return replacement

    def method(name):
        orig, copy = o_me[name], name in INITIALISING

        def replacement(self, *args, **kw):
            return house(orig(self, *args, **kw), name, copy)

        def operand(self, *args, **kw):
            r = orig(self, *args, **kw)
            if r is self or not isinstance(self, torch.Tensor) or self.device.type != 'cpu' or not isinstance(r, torch.Tensor) or not r.is_cuda \
                    or r.grad_fn is not None or r.requires_grad:
                return r
            return house(r, name, True)
        chosen = operand if name in OPERANDS else replacement
        chosen.__name__ = name
        return chosen

    alloc_fill._active[0] = rec
    try:
        for n in _FUNCTIONS:
            setattr(torch, n, function(n))
        for n in methods:
            setattr(torch.Tensor, n, method(n))
        yield rec
    finally:
        for n in _FUNCTIONS:
            setattr(torch, n, o_fn[n])
        for n in methods:
            if own[n]:
                setattr(torch.Tensor, n, o_me[n])
            elif n in vars(torch.Tensor):
                delattr(torch.Tensor, n)
        alloc_fill._active[0] = None
        rec.closed = True
        for a in rec.allocations:
            a.raw = None
