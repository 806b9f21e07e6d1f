"""Training statistics on the device: what ``training_stats.report`` / ``Collector`` of the StyleGAN2-ADA code base do for the reference's
training loop (``lib/experiments/stylegan_default.py:408-422, :540-557``), on one kernel (``shg_stats_moments_f64``, csrc/train_stats.hip).

A ``Collector`` owns ``acc``, a float64 ``[slots, 4]`` table on the device with the columns {count, sum, sum of squares, non-finite count};
a name gets its slot at first sight.  ``report`` / ``report_many`` make ONE launch per call, whatever the number of tensors: the call's
tensors travel as a small int64 table ``[rows + 1, 4]`` = {address, numel, slot, 0}.  Nothing is read back until ``update()``: one
all-reduce of the whole table when ``torch.distributed`` is initialised, one device-to-host copy through pinned memory, then the table
is reset.  ``as_dict()`` is host arithmetic on that copy.

Graph capture: a captured launch reads its table block on every replay, so the block (pinned host words, device words and the copy
between them) is cut from a pool the collector allocates at construction, filled once at capture and never written again.  A name or a row shape that no eager call has shown raises under capture, as ``optim.ShgAdam._table`` does.

There is no fallback: device tensors go through the kernel.  ``accumulate_fn`` replaces the launch as a whole (``Inpainter(gather_fn=...)``
is the pattern): the host logic then runs anywhere, e.g. on the CPU with the float64 numpy yardstick of the tests."""
import ctypes
import math

import numpy as np
import torch

from . import _lib, kernels
from ._lib import ShgError, check

STATS_ROW = 4         # csrc/train_stats.hip STATS_ROW: {address, numel, slot, 0}
STATS_COLS = 4        # {count, sum, sum of squares, non-finite count}
MAX_SLOTS = 1024


def build_stats_table(rows):
    """rows: (address, numel, slot) -> int64 [len(rows) + 1, STATS_ROW], the sentinel row last ({0, 0, -1, 0})."""
    tab = np.zeros((len(rows) + 1, STATS_ROW), np.int64)
    for i, (addr, n, slot) in enumerate(rows):
        tab[i] = (addr, n, slot, 0)
    tab[-1, 2] = -1
    return tab


def validate_stats_table(tab, slots, extents=None):
    """Every row a whole, aligned float32 tensor and a slot of the table: raises ShgError, before any launch.  ``extents``: (address, bytes)
    of the allocations a row may read (None: not checked)."""
    tab = np.asarray(tab)
    if tab.ndim != 2 or tab.shape[1] != STATS_ROW or tab.shape[0] < 1 or tab.dtype != np.int64:
        raise ShgError('stats table: int64 [rows + 1, %d] expected' % STATS_ROW)
    if tuple(tab[-1].tolist()) != (0, 0, -1, 0):
        raise ShgError('stats table: the last row must be the sentinel {0, 0, -1, 0}')
    for i, (addr, n, slot, zero) in enumerate(tab[:-1].tolist()):
        if n < 1:
            raise ShgError(f'stats table: row {i} has {n} elements')
        if addr <= 0 or addr % 4:
            raise ShgError(f'stats table: row {i} is misaligned (a 4-byte aligned address expected, got {addr:#x})')
        if not 0 <= slot < slots:
            raise ShgError(f'stats table: row {i} names slot {slot} of {slots}')
        if zero != 0:
            raise ShgError(f'stats table: row {i} has a non-zero last column')
        if extents is not None and not any(a0 <= addr and addr + 4 * n <= a0 + nb for a0, nb in extents):
            raise ShgError(f'stats table: row {i} leaves its tensor')
    return tab


def _check_tensor(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'Collector: {name!r} is not a tensor (host numbers go through report0)')
    if t.dtype != torch.float32:
        raise ShgError(f'Collector: {name!r} is {t.dtype}; float32 tensors only')
    if not t.is_contiguous():
        raise ShgError(f'Collector: {name!r} is not contiguous')
    if t.numel() < 1:
        raise ShgError(f'Collector: {name!r} is empty')


def _pinned_zeros(shape, dtype):
    """A zeroed HOST staging block in pinned memory (device buffers come from ``kernels._Launch.new``)."""
    return torch.from_numpy(np.zeros(tuple(shape), dtype)).pin_memory()


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class Collector:
    """See the module docstring.  ``device``: where ``acc`` lives (the tensors reported must be there).  ``slots``: capacity of the table
    (names; fixed, because captured launches hold its address).  ``capture_words``: size (int64 words) of the pool the table blocks of
    captured launches are cut from -- a block of rows + 1 rows of 4 words per captured ``report_many``; the pool is never grown, because
    captured launches hold addresses inside it."""

    def __init__(self, device, slots=64, accumulate_fn=None, process_group=None, capture_words=1 << 14):
        self.device = torch.device(device)
        if not 1 <= int(slots) <= MAX_SLOTS:
            raise ValueError(f'Collector: slots in [1, {MAX_SLOTS}]')
        self.slots = int(slots)
        launch = kernels._Launch()       # (``launch``, not ``L``: the allocation tests cover this class from tests/test_gpu_train_run.py)
        launch.dev = self.device
        self.acc = launch.new([self.slots, STATS_COLS], torch.float64).zero_()
        self.names = {}                # name -> slot
        self.launches = 0
        self.collectives = 0
        self.accumulate_fn = accumulate_fn
        self.group = process_group
        self._host0 = {}               # name -> [count, sum, sum of squares] of report0 since the last update
        self._totals = np.zeros([self.slots, STATS_COLS], np.float64)      # what the last update() read
        self._seen = set()             # (names, numels) of the eager calls: what a capture may repeat
        # the blocks captured launches read: cut from this pair (pinned host words, device words), filled once at capture, never written
        # again.  Allocated here, not under capture (pinned memory cannot be allocated there)
        self._pool_used = 0
        self._pool = None
        if self.device.type == 'cuda' and accumulate_fn is None:
            self._pool = (_pinned_zeros([int(capture_words)], np.int64), launch.new([int(capture_words)], torch.int64).zero_())
        self._pin = None

    # -- bookkeeping ---------------------------------------------------------------------------------------------------------------------
    def _slot(self, name):
        slot = self.names.get(name)
        if slot is None:
            if _capturing():
                raise RuntimeError(f'Collector: the name {name!r} was not seen before the graph capture; report it in an eager call first')
            if len(self.names) >= self.slots:
                raise ShgError(f'Collector: more than {self.slots} names (build the collector with more slots)')
            slot = self.names[name] = len(self.names)
        return slot

    def host_table(self, tensors):
        """The (validated) table of one call: ``tensors`` is {name: tensor}."""
        rows, extents = [], []
        for name, t in tensors.items():
            _check_tensor(name, t)
            if t.device != self.device:
                raise ShgError(f'Collector: {name!r} lives on {t.device}, the collector on {self.device}')
            rows.append((t.data_ptr(), t.numel(), self._slot(name)))
            extents.append((t.data_ptr(), 4 * t.numel()))
        return validate_stats_table(build_stats_table(rows), self.slots, extents)

    # -- reporting -----------------------------------------------------------------------------------------------------------------------
    def report(self, name, tensor):
        self.report_many({name: tensor})
        return tensor

    def report_many(self, tensors):
        """One launch for all of ``tensors`` ({name: float32 tensor}); an empty dict launches nothing."""
        if not tensors:
            return
        if _capturing():
            unseen = [n for n in tensors if n not in self.names]
            if unseen:
                raise RuntimeError(f'Collector: the name {unseen[0]!r} was not seen before the graph capture; report it in an eager call first')
        tab = self.host_table(tensors)
        if self.accumulate_fn is not None:
            self.accumulate_fn(tab, self.acc, tensors)
            self.launches += 1
            return
        if self.device.type != 'cuda':
            raise ShgError('Collector: tensors must live on a HIP device: libshgan_hip has no CPU path (pass accumulate_fn for host-side use)')
        key = (tuple(tensors), tuple(int(t.numel()) for t in tensors.values()))
        if _capturing():
            if key not in self._seen:
                raise RuntimeError('Collector: these names and row shapes were not reported in an eager call before the graph capture: '
                                   f'{list(tensors)}')
            words = tab.size
            if self._pool_used + words > self._pool[0].numel():
                raise RuntimeError(f'Collector: the pool of table blocks for captured launches is used up ({self._pool[0].numel()} words); '
                                   'build the collector with a larger capture_words')
            host = self._pool[0][self._pool_used:self._pool_used + words]
            dev = self._pool[1][self._pool_used:self._pool_used + words]
            self._pool_used += words
            host.copy_(torch.from_numpy(tab).reshape(-1))        # plain host write; the copy below is a node of the graph
            dev.copy_(host, non_blocking=True)
        else:
            self._seen.add(key)
            dev = torch.from_numpy(tab).pin_memory().to(self.device, non_blocking=True)
        with torch.cuda.device(self.device):
            check(_lib.get_lib().shg_stats_moments_f64(ctypes.c_void_p(dev.data_ptr()), tab.shape[0] - 1, ctypes.c_void_p(self.acc.data_ptr()),
                                                       self.slots, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                  'stats_moments_f64')
        self.launches += 1

    def report0(self, name, value):
        """A host number: same bookkeeping, no launch."""
        self._slot(name)
        v = float(value)
        h = self._host0.setdefault(name, [0.0, 0.0, 0.0, 0.0])
        if math.isfinite(v):
            h[0] += 1.0
            h[1] += v
            h[2] += v * v
        else:
            h[3] += 1.0
        return value

    # -- the tick's read-back ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self):
        """All-reduce (when distributed), ONE device-to-host copy of ``acc``, reset.  Host numbers of ``report0`` are this rank's."""
        if _capturing():
            raise RuntimeError('Collector.update() reads back: call it outside a graph capture')
        acc = self.acc
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            backend = torch.distributed.get_backend(self.group)
            buf = acc if (backend == 'nccl') == (acc.device.type == 'cuda') else acc.to('cuda' if backend == 'nccl' else 'cpu')
            torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.SUM, group=self.group)
            self.collectives += 1
            if buf is not acc:
                acc.copy_(buf)
        if acc.device.type == 'cuda':
            if self._pin is None:
                self._pin = _pinned_zeros(acc.shape, np.float64)
            self._pin.copy_(acc, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            host = self._pin.numpy().copy()
        else:
            host = acc.numpy().copy()
        acc.zero_()
        for name, h in self._host0.items():
            host[self.names[name]] += np.asarray(h, np.float64)
        self._host0 = {}
        self._totals = host
        return self

    def totals(self):
        """float64 [slots, 4] of the last ``update()``."""
        return self._totals.copy()

    def as_dict(self):
        """{name: {'num', 'mean', 'std'}} of the last ``update()`` (+ 'nonfinite' where elements were not finite)."""
        out = {}
        for name, slot in self.names.items():
            cnt, s, ss, bad = (float(v) for v in self._totals[slot])
            if cnt == 0:
                d = {'num': 0, 'mean': float('nan'), 'std': float('nan')}
            else:
                mean = s / cnt
                d = {'num': int(cnt), 'mean': mean, 'std': math.sqrt(max(ss / cnt - mean * mean, 0.0))}
            if bad != 0:
                d['nonfinite'] = int(bad)
            out[name] = d
        return out

    def __getitem__(self, name):
        return self.as_dict()[name]['mean']
