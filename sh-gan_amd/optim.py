"""The tail of a training iteration on this library's kernels (csrc/optim.hip): Adam over the gradient buckets and the G_ema update.

The reference's iteration ends with ``nan_to_num`` over every gradient, ``opt.step()`` (``torch.optim.Adam``) and a per-parameter
``p_ema.copy_(p.lerp(p_ema, beta))`` loop (``lib/experiments/stylegan_default.py:159-166, :383-390``).  Here
  * ``ShgAdam`` reads the gradients where the all-reduce left them -- the flat buckets of ``grad_sync.BucketedAllReduce`` -- and does
    the average over the ranks, the sanitisation and the Adam update in ONE pass (``shg_adam_buckets_f32``), after a one-workgroup
    kernel that advances the per-parameter step counters and computes the bias corrections on the device (``shg_adam_tick``): no host
    read, so the step can be captured in a HIP graph.  ``exp_avg`` / ``exp_avg_sq`` live in flat buffers laid out like the buckets.
  * ``EmaUpdater`` updates every parameter and buffer of ``G_ema`` in one launch (``shg_ema_lerp_f32``); beta is read from a device
    slot, so a captured launch follows ``ema_rampup``.
Both keep torch's float32 arithmetic (``lerp`` in its two forms, the reciprocal ``div_`` of a host scalar): see the kernels.  There is no
fallback: an option the kernels do not implement raises, a CPU tensor raises at the first step."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ShgError, check
from .grad_sync import BucketedAllReduce

CHUNK = 4096          # csrc/optim.hip OPT_CHUNK
ADAM_ROW = 10         # {param, grad, exp_avg, exp_avg_sq, numel, touched, scalar slot, group, 0, first chunk}
EMA_ROW = 6           # {dst, src, words, kind, 0, first chunk}
ADAM_SCALARS = 8
EMA_LERP, EMA_COPY = 0, 1
DIV_NONE, DIV_RECIPROCAL, DIV_TRUE = 0, 1, 2
HEALTH_COLS = 5       # csrc/optim.hip HEALTH_COLS: {sum g^2, elements the sanitisation replaced, max |g|, sum p_old^2, sum (p_old - p_new)^2}


def _chunk_prefix(numels):
    """first chunk of every segment, then the total: a segment of n elements has ceil(n / CHUNK) chunks."""
    counts = [-(-int(n) // CHUNK) for n in numels]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def build_adam_table(segments, bases, touched=None):
    """segments: per parameter (param address, bucket index, offset in the bucket, numel, scalar slot, group); bases: per bucket
    (gradient, exp_avg, exp_avg_sq base addresses, numel of the bucket); touched: the scalar slots that received a gradient (None: all).
    -> int64 [len(segments) + 1, ADAM_ROW], rows in the given order, the sentinel row last."""
    tab = np.zeros((len(segments) + 1, ADAM_ROW), np.int64)
    start = _chunk_prefix([s[3] for s in segments])
    for i, (p_addr, bi, off, n, slot, grp) in enumerate(segments):
        if not 0 <= bi < len(bases):
            raise ShgError(f'adam table: segment {i} names bucket {bi} of {len(bases)}')
        g0, m0, v0, _ = bases[bi]
        tab[i] = (p_addr, g0 + 4 * off, m0 + 4 * off, v0 + 4 * off, n, 1 if touched is None or slot in touched else 0, slot, grp, 0, start[i])
    tab[-1, -1] = start[-1]
    return tab


def validate_adam_table(tab, bases, n_slots, n_groups):
    """Every row inside its bucket, slots distinct and in range, the chunk column consistent: raises ShgError, before any launch."""
    tab = np.asarray(tab)
    if tab.ndim != 2 or tab.shape[1] != ADAM_ROW or tab.shape[0] < 2 or tab.dtype != np.int64:
        raise ShgError('adam table: int64 [segments + 1, %d] expected' % ADAM_ROW)
    rows = tab[:-1]
    seen = set()
    for i, (p, g, m, v, n, t, slot, grp, _, c0) in enumerate(rows.tolist()):
        if n < 1:
            raise ShgError(f'adam table: segment {i} has {n} elements')
        if p <= 0 or p % 4 or g % 4 or (g - m) % 16 or (g - v) % 16:
            raise ShgError(f'adam table: segment {i} is misaligned (4-byte addresses; gradient and moments congruent mod 16)')
        if not any(g0 <= g and g + 4 * n <= g0 + 4 * nb and m - m0 == g - g0 and v - v0 == g - g0 for g0, m0, v0, nb in bases):
            raise ShgError(f'adam table: segment {i} (offset + numel) leaves its bucket')
        if not 0 <= slot < n_slots or slot in seen:
            raise ShgError(f'adam table: segment {i} has scalar slot {slot} (of {n_slots}, each used once)')
        seen.add(slot)
        if not 0 <= grp < n_groups:
            raise ShgError(f'adam table: segment {i} names hyper-parameter group {grp} of {n_groups}')
        if t not in (0, 1):
            raise ShgError(f'adam table: segment {i} has touched flag {t}')
    if not np.array_equal(tab[:, -1], _chunk_prefix(rows[:, 4])):
        raise ShgError('adam table: the chunk column is not the prefix sum of ceil(numel / %d)' % CHUNK)
    return tab


def build_ema_table(pairs):
    """pairs: (dst address, src address, 32-bit words, kind) -> int64 [len(pairs) + 1, EMA_ROW]."""
    tab = np.zeros((len(pairs) + 1, EMA_ROW), np.int64)
    start = _chunk_prefix([q[2] for q in pairs])
    for i, (d, s, n, kind) in enumerate(pairs):
        tab[i] = (d, s, n, kind, 0, start[i])
    tab[-1, -1] = start[-1]
    return tab


def validate_ema_table(tab, extents):
    """extents: (address, bytes) of every allocation a row may touch.  Raises ShgError on a row that leaves them, before any launch."""
    tab = np.asarray(tab)
    if tab.ndim != 2 or tab.shape[1] != EMA_ROW or tab.shape[0] < 2 or tab.dtype != np.int64:
        raise ShgError('ema table: int64 [segments + 1, %d] expected' % EMA_ROW)

    def inside(a, nbytes):
        return any(a0 <= a and a + nbytes <= a0 + nb for a0, nb in extents)
    for i, (d, s, n, kind, _, c0) in enumerate(tab[:-1].tolist()):
        if n < 1 or kind not in (EMA_LERP, EMA_COPY) or d <= 0 or s <= 0 or d % 4 or s % 4:
            raise ShgError(f'ema table: segment {i} is malformed (words {n}, kind {kind}, 4-byte addresses)')
        if not inside(d, 4 * n) or not inside(s, 4 * n):
            raise ShgError(f'ema table: segment {i} leaves its tensor')
    if not np.array_equal(tab[:, -1], _chunk_prefix(tab[:-1, 2])):
        raise ShgError('ema table: the chunk column is not the prefix sum of ceil(words / %d)' % CHUNK)
    return tab


def _upload(host, like_device, out=None):
    """Host array -> device tensor through pinned memory, asynchronous on the current stream (the pinned block is kept by the caching host
    allocator until the copy has run)."""
    t = torch.from_numpy(np.ascontiguousarray(host))
    t = t.pin_memory() if like_device.type == 'cuda' else t
    if out is None:
        return t.to(like_device, non_blocking=True)
    out.copy_(t, non_blocking=True)
    return out


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _bump_versions(tensors):
    """The kernels write behind autograd's back: move the version counters so that everything keyed on them (prepared weight layouts of
    ``model_zoo.stylegan._ParamCache``, a watching ``GraphPipeline``) sees the write."""
    tensors = list(tensors)
    if tensors:
        torch._C._increment_version(tensors)


class ShgAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (weight_decay 0, amsgrad off) on the gradient buckets.

    ``sync``: the ``BucketedAllReduce`` whose layout is shared -- every parameter of the optimiser must be in it; ``None`` builds
    private buckets of ``bucket_bytes``.  ``step_from_buckets(reduced)`` replaces ``sync.finish(reduced)`` + ``p.grad = None`` for the
    untouched + ``opt.step()``; ``step()`` is the same call with ``reduced=False``.
    A parameter that received no gradient since ``sync.zero_grad()`` keeps its value, its moments and its step counter bit for bit
    (``zero_grad(set_to_none=True)`` semantics).
    Raises for ``weight_decay != 0``, ``amsgrad``, ``maximize``, ``differentiable``, ``foreach`` / ``fused`` requests, tensor ``lr`` and
    parameters that are not contiguous float32.  ``capturable`` is only recorded in the param groups (for a torch optimiser that loads
    this one's state): the step counter is on the device either way.
    ``lr`` / ``betas`` / ``eps`` of a group may be changed between eager steps (the device block is refreshed at the next step); a
    captured step replays with the values it was captured with, like torch's capturable Adam.
    ``state_dict()`` / ``load_state_dict()`` use ``torch.optim.Adam``'s layout (per-parameter ``step``, ``exp_avg``, ``exp_avg_sq``).
    ``health=True``: the step is ``shg_adam_buckets_health_f32`` + ``shg_health_reduce_f64`` -- the same pass with the same bits in every
    parameter and moment, which also leaves gradient-health figures of the values it read anyway in ``health_table()``, float64
    ``[parameters + 1, HEALTH_COLS]`` on the device (row i = ``_params[i]``, the last row the optimiser's total): sums added and the
    maximum kept over the steps since ``health_reset()``; no host read, capturable.  Off by default: the plain entry point."""

    DIV_MODE = DIV_RECIPROCAL      # how the average is taken for world > 1: as torch's div_ by a host scalar does on the device

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None, sync=None, bucket_bytes=64 << 20, health=False):
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults)       # torch's keys, whatever the version
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=bool(capturable), differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)
        self._check_groups()
        plist = [p for g in self.param_groups for p in g['params']]
        if not plist:
            raise ValueError('ShgAdam: no parameters')
        for p in plist:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise TypeError('ShgAdam: contiguous float32 parameters only')
        self._own_sync = sync is None
        self.sync = BucketedAllReduce(plist, bucket_bytes=bucket_bytes) if sync is None else sync
        try:
            slots = [self.sync.slot(p) for p in plist]
        except KeyError:
            raise ValueError('ShgAdam: a parameter is not in the gradient buckets of `sync`') from None
        self.device = plist[0].device
        if any(p.device != self.device for p in plist):
            raise ValueError('ShgAdam: all parameters on one device')
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g['params']}
        order = sorted(range(len(plist)), key=lambda i: slots[i][:2])             # streaming order: bucket by bucket, ascending offsets
        self._params = [plist[i] for i in order if plist[i].numel() > 0]
        self._segs = [(self.sync.slot(p), group_of[id(p)]) for p in self._params]
        self._slot_of = {id(p): i for i, p in enumerate(self._params)}
        self.exp_avg = [torch.zeros_like(b) for b in self.sync.buckets]
        self.exp_avg_sq = [torch.zeros_like(b) for b in self.sync.buckets]
        n = len(self._params)
        self.steps = torch.zeros(n, dtype=torch.float32, device=self.device)
        self._scalars = torch.zeros(n * ADAM_SCALARS, dtype=torch.float32, device=self.device)
        self._hyper = torch.zeros(len(self.param_groups) * 4, dtype=torch.float64, device=self.device)
        self._hyper_host = None
        self._tables = {}               # touched set -> (device table, chunks)
        self.health = bool(health)
        if self.health:                 # allocated here: a captured step holds the addresses
            chunks = int(_chunk_prefix([p.numel() for p in self._params])[-1])
            self._health_ws = torch.zeros([chunks, HEALTH_COLS], dtype=torch.float64, device=self.device)
            self._health = torch.zeros([n + 1, HEALTH_COLS], dtype=torch.float64, device=self.device)
            self._health_steps = torch.zeros([1], dtype=torch.float64, device=self.device)
        self._attach_state()

    # -- hyper-parameters ------------------------------------------------------------------------------------------------------------
    def _check_groups(self):
        for g in self.param_groups:
            if isinstance(g['lr'], torch.Tensor):
                raise ValueError('ShgAdam: lr must be a number (the kernels read it from their own device block)')
            if g.get('weight_decay', 0) != 0:
                raise ValueError('ShgAdam: weight_decay is not implemented (the reference trains with 0)')
            for k in ('amsgrad', 'maximize', 'differentiable'):
                if g.get(k, False):
                    raise ValueError(f'ShgAdam: {k} is not implemented')
            for k in ('foreach', 'fused'):
                if g.get(k) is not None and g.get(k) is not False:
                    raise ValueError(f'ShgAdam: {k} selects a torch implementation; this optimiser has one HIP kernel')
            b1, b2 = g['betas']
            if not (g['lr'] >= 0 and g['eps'] >= 0 and 0 <= b1 < 1 and 0 <= b2 < 1):
                raise ValueError(f'ShgAdam: invalid lr / betas / eps {g["lr"]}, {g["betas"]}, {g["eps"]}')

    def _sync_hyper(self):
        self._check_groups()
        host = tuple(float(x) for g in self.param_groups for x in (g['lr'], g['betas'][0], g['betas'][1], g['eps']))
        if host != self._hyper_host:
            if _capturing():
                raise RuntimeError('ShgAdam: hyper-parameters changed inside a graph capture; run one eager step first')
            _upload(np.asarray(host, np.float64), self.device, out=self._hyper)
            self._hyper_host = host

    # -- state -----------------------------------------------------------------------------------------------------------------------
    def _views(self, p):
        (bi, off, n), _ = self._segs[self._slot_of[id(p)]]
        i = self._slot_of[id(p)]
        return self.steps[i], self.exp_avg[bi][off:off + n].view_as(p), self.exp_avg_sq[bi][off:off + n].view_as(p)

    def _attach_state(self):
        self.state.clear()
        for p in self._params:
            st, m, v = self._views(p)
            self.state[p] = {'step': st, 'exp_avg': m, 'exp_avg_sq': v}

    def state_dict(self):
        """torch.optim.Adam's layout; the tensors are copies (a checkpoint does not drag the flat buffers along)."""
        sd = super().state_dict()
        sd['state'] = {k: {n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in st.items()} for k, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        """From this class or from ``torch.optim.Adam`` (``step`` as a tensor on any device or as a number; parameters without an entry
        start from zero state)."""
        super().load_state_dict(state_dict)
        self._check_groups()
        loaded = dict(self.state)
        with torch.no_grad():
            for p in self._params:
                st, m, v = self._views(p)
                got = loaded.get(p)
                if not got:
                    st.zero_(), m.zero_(), v.zero_()
                    continue
                if 'max_exp_avg_sq' in got:
                    raise ValueError('ShgAdam: the state was saved with amsgrad')
                step = got['step']
                st.fill_(float(step.item() if isinstance(step, torch.Tensor) else step))
                m.copy_(got['exp_avg'])
                v.copy_(got['exp_avg_sq'])
        self._attach_state()
        self._hyper_host = None

    # -- tables ----------------------------------------------------------------------------------------------------------------------
    def host_table(self, touched_ids=None):
        """The (validated) segment table for a set of ``id(p)`` (None: every parameter)."""
        bases = [(g.data_ptr(), m.data_ptr(), v.data_ptr(), g.numel()) for g, m, v in zip(self.sync.buckets, self.exp_avg, self.exp_avg_sq)]
        segs = [(p.data_ptr(), bi, off, n, i, grp) for i, (p, ((bi, off, n), grp)) in enumerate(zip(self._params, self._segs))]
        touched = None if touched_ids is None else {self._slot_of[i] for i in touched_ids if i in self._slot_of}
        return validate_adam_table(build_adam_table(segs, bases, touched), bases, len(self._params), len(self.param_groups))

    def _table(self, touched_ids):
        key = (touched_ids, tuple(p.data_ptr() for p in self._params))
        hit = self._tables.get(key)
        if hit is None:
            if _capturing():
                raise RuntimeError('ShgAdam: this set of parameters with gradients was not seen before the graph capture; run the phase '
                                   'eagerly first (PhaseGraphs warm-up) so that its segment table is on the device')
            tab = self.host_table(touched_ids)
            hit = self._tables[key] = (_upload(tab, self.device), int(tab[-1, -1]))
        return hit

    # -- the step --------------------------------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        if self._own_sync:
            self.sync.zero_grad()
        else:
            super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.step_from_buckets(reduced=False)
        return loss

    @torch.no_grad()
    def step_from_buckets(self, reduced=False, world=None):
        """``sync.finish(reduced)`` + the optimiser step, in two launches.  ``world``: the divisor of the average (default: the group's
        size); afterwards the buckets hold the averaged, sanitised gradients, untouched parameters have ``grad = None`` and ``sync`` is
        re-armed, as after ``finish()``."""
        sync = self.sync
        if self.device.type != 'cuda':
            raise ShgError('ShgAdam: parameters must live on a HIP device: libshgan_hip has no CPU path')
        sync.complete(reduced=reduced)
        touched = sync.touched_ids()
        self._sync_hyper()
        tab, chunks = self._table(touched)
        world = sync.world if world is None else int(world)
        lib = _lib.get_lib()
        nseg = len(self._params)
        with torch.cuda.device(self.device):
            st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(lib.shg_adam_tick(ctypes.c_void_p(tab.data_ptr()), nseg, ctypes.c_void_p(self._hyper.data_ptr()), len(self.param_groups),
                                    ctypes.c_void_p(self.steps.data_ptr()), ctypes.c_void_p(self._scalars.data_ptr()), st), 'adam_tick')
            if self.health:
                if chunks != self._health_ws.shape[0]:
                    raise ShgError(f'ShgAdam: the table has {chunks} chunks, the health workspace {self._health_ws.shape[0]}')
                check(lib.shg_adam_buckets_health_f32(ctypes.c_void_p(tab.data_ptr()), nseg, chunks, ctypes.c_void_p(self._scalars.data_ptr()),
                                                      float(world), self.DIV_MODE if world > 1 else DIV_NONE, int(bool(sync.sanitize)),
                                                      ctypes.c_void_p(self._health_ws.data_ptr()), st), 'adam_buckets_health_f32')
                check(lib.shg_health_reduce_f64(ctypes.c_void_p(tab.data_ptr()), nseg, chunks, ctypes.c_void_p(self._health_ws.data_ptr()),
                                                ctypes.c_void_p(self._health.data_ptr()), ctypes.c_void_p(self._health_steps.data_ptr()), st),
                      'health_reduce_f64')
            else:
                check(lib.shg_adam_buckets_f32(ctypes.c_void_p(tab.data_ptr()), nseg, chunks, ctypes.c_void_p(self._scalars.data_ptr()),
                                               float(world), self.DIV_MODE if world > 1 else DIV_NONE, int(bool(sync.sanitize)), st),
                      'adam_buckets_f32')
        sync.rearm()
        for p in sync.untouched():             # as after zero_grad(set_to_none=True)
            p.grad = None
        _bump_versions(p for p in self._params if id(p) in touched)

    # -- gradient health (health=True) -----------------------------------------------------------------------------------------------
    def _need_health(self):
        if not self.health:
            raise ShgError('ShgAdam: built with health=False: there is no health table')

    def health_table(self):
        """float64 [parameters + 1, HEALTH_COLS] on the device (the tensor the kernels write, not a copy)."""
        self._need_health()
        return self._health

    def health_steps(self):
        """float64 [1] on the device: the steps (with at least one gradient) since the last reset."""
        self._need_health()
        return self._health_steps

    @torch.no_grad()
    def health_reset(self):
        self._need_health()
        self._health.zero_()
        self._health_steps.zero_()

    @torch.no_grad()
    def health_report(self, collector, prefix):
        """The optimiser's totals since the last reset as one value each in the collector's slots ``Grad/<prefix>/norm`` (root of the mean
        over the steps of sum g^2), ``Grad/<prefix>/nonfinite`` (elements the sanitisation replaced), ``Grad/<prefix>/max`` (largest |g|) and
        ``Update/<prefix>/ratio`` (sqrt(sum dp^2) / sqrt(sum p^2)); then the table is reset.  A few small device operations and one collector
        launch, no host read; nothing is reported when no step was taken.  Call it once per tick, outside graph captures.  The collector
        takes float32 tensors, so each total is rounded to float32 once on its way in: a count of replaced elements above 2^24 is then
        within 6e-8 of itself, no longer exact (``health_table()`` / ``health_rows()`` keep the float64 value)."""
        self._need_health()
        tot, steps = self._health[-1], self._health_steps[0].clamp(min=1.0)
        vals = torch.stack([(tot[0] / steps).sqrt(), tot[1], tot[2], (tot[4] / tot[3].clamp(min=1e-300)).sqrt()]).to(torch.float32)
        collector.report_many({f'Grad/{prefix}/norm': vals[0:1], f'Grad/{prefix}/nonfinite': vals[1:2], f'Grad/{prefix}/max': vals[2:3],
                               f'Update/{prefix}/ratio': vals[3:4]})
        self.health_reset()

    def health_rows(self, names=None):
        """{name: {'grad_sq', 'nonfinite', 'grad_max', 'param_sq', 'update_sq'}} per parameter since the last reset (one read-back).
        ``names``: {id(p): name}, e.g. from ``module.named_parameters()``; default: the index in streaming order."""
        self._need_health()
        host = self._health.cpu().numpy()
        keys = ('grad_sq', 'nonfinite', 'grad_max', 'param_sq', 'update_sq')
        out = {}
        for i, p in enumerate(self._params):
            name = str(i) if names is None else names.get(id(p), str(i))
            out[name] = dict(zip(keys, (float(v) for v in host[i])))
        out['total'] = dict(zip(keys, (float(v) for v in host[-1])))
        return out


class EmaUpdater:
    """``train_stage.update_ema`` in one launch: ``p_ema = lerp(p, p_ema, beta)`` for the parameters, a bitwise copy for the buffers.

    The table is built once (the tensors of both networks must stay where they are).  ``update()`` = ``set_beta()`` + ``launch()`` +
    new version counters for what was written (so ``G_ema``'s prepared weight layouts are rebuilt); ``launch()`` alone is what a HIP graph captures -- ``capture()`` does that, and ``update()`` then replays it after
    writing the new beta to the device slot, so one captured launch follows ``ema_rampup``."""

    def __init__(self, G_ema, G):
        pe, ps = list(G_ema.parameters()), list(G.parameters())
        be, bs = list(G_ema.buffers()), list(G.buffers())
        if len(pe) != len(ps) or len(be) != len(bs):
            raise ValueError('EmaUpdater: G_ema and G differ in their parameters / buffers')
        pairs, extents, self._written = [], [], []
        for kind, dsts, srcs in ((EMA_LERP, pe, ps), (EMA_COPY, be, bs)):
            for d, s in zip(dsts, srcs):
                if d.shape != s.shape or d.dtype != s.dtype or d.device != s.device or not d.is_contiguous() or not s.is_contiguous():
                    raise ValueError('EmaUpdater: tensors of G_ema and G must agree in shape, dtype and device and be contiguous')
                if kind == EMA_LERP and d.dtype != torch.float32:
                    raise TypeError('EmaUpdater: float32 parameters only')
                nbytes = d.numel() * d.element_size()
                if nbytes % 4 or d.data_ptr() % 4 or s.data_ptr() % 4:
                    raise TypeError('EmaUpdater: a buffer is not a whole number of aligned 32-bit words')
                if nbytes == 0:
                    continue
                pairs.append((d.data_ptr(), s.data_ptr(), nbytes // 4, kind))
                extents += [(d.data_ptr(), nbytes), (s.data_ptr(), nbytes)]
                self._written.append(d)
        if not pairs:
            raise ValueError('EmaUpdater: nothing to update')
        self.device = self._written[0].device
        if any(t.device != self.device for t in self._written):
            raise ValueError('EmaUpdater: all tensors on one device')
        self.host_table = validate_ema_table(build_ema_table(pairs), extents)
        self._nseg, self._chunks = len(pairs), int(self.host_table[-1, -1])
        self._tab = self._slot = self._graph = None

    def _ready(self):
        if self.device.type != 'cuda':
            raise ShgError('EmaUpdater: the networks must live on a HIP device: libshgan_hip has no CPU path')
        if self._tab is None:
            if _capturing():
                raise RuntimeError('EmaUpdater: call set_beta() once before capturing launch()')
            self._tab = _upload(self.host_table, self.device)
            self._slot = torch.zeros(1, dtype=torch.float32, device=self.device)

    def set_beta(self, beta):
        """Write beta to the device slot (pinned host memory, asynchronous, in stream order before the next launch / replay)."""
        self._ready()
        if _capturing():
            raise RuntimeError('EmaUpdater.set_beta() is a host-to-device copy: call it before the replay, capture launch() only')
        _upload(np.asarray([beta], np.float32), self.device, out=self._slot)

    def launch(self):
        """The one kernel launch, on the current stream (capturable)."""
        self._ready()
        with torch.cuda.device(self.device):
            check(_lib.get_lib().shg_ema_lerp_f32(ctypes.c_void_p(self._tab.data_ptr()), self._nseg, self._chunks,
                                                  ctypes.c_void_p(self._slot.data_ptr()),
                                                  ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), 'ema_lerp_f32')

    def capture(self):
        """Record ``launch()`` as a HIP graph; ``update()`` replays it from now on."""
        self._ready()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.launch()
        self._graph = g
        return g

    @torch.no_grad()
    def update(self, batch_size, cur_nimg, ema_kimg=10.0, ema_rampup=None):
        from .train_stage import ema_beta
        beta = ema_beta(batch_size, cur_nimg, ema_kimg, ema_rampup)
        self.set_beta(beta)
        if self._graph is not None:
            self._graph.replay()
        else:
            self.launch()
        _bump_versions(self._written)          # G_ema's prepared weight layouts are keyed on the version counters
        return beta
