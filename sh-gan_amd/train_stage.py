"""The training stage around the G / D step: phases with lazy regularisation, the per-iteration phase
loop, gradient sanitisation + all-reduce, the G_ema update.

Mirrors ``lib/experiments/stylegan_default.py``:
  * ``make_phases``  -- :304-321.  One optimiser per network; with a regularisation interval r the 'main' phase runs every
    iteration and the 'reg' phase every r-th, and the optimiser's hyper-parameters absorb the skipped steps
    (``mb_ratio = r / (r + 1)``, ``lr * mb_ratio``, ``beta ** mb_ratio``); without one a single 'both' phase.
  * ``run_phases``   -- ``train_stage.main`` :108-167: the latents of all phases drawn at once, every phase whose interval divides the
    iteration index zeroes its gradients, opens ``requires_grad`` on ITS module only, accumulates over the rounds of
    ``effective_batch_gpu`` samples (``loss.accumulate_gradients(phase, real_img, real_c, gen_z, gen_c, sync, gain=interval)``),
    sanitises the gradients (``nan_to_num(nan=0, posinf=1e5, neginf=-1e5)``) and steps.
  * ``update_ema``   -- :383-390: ``ema_beta = 0.5 ** (batch_size / max(ema_nimg, 1e-8))`` with the ``ema_rampup`` cap, buffers copied.
  * ``train``        -- the iteration loop :370-396; its logging / snapshot / metric maintenance (the tick block :402-575) is opt-in:
    ``Maintenance`` (status line, metrics, sample grid, snapshot, ``stats.jsonl``), ``save_snapshot`` / ``load_snapshot`` (state_dicts,
    counters and RNG states: a resumed run continues with the bits of the uninterrupted one) and ``image_grid``
    (``draw_functor.output`` :74-84 on the device).  ``on_tick`` stays the hook for anything else.
The reference wraps the networks in DistributedDataParallel (:172-187); here every phase owns a ``grad_sync.BucketedAllReduce`` over
its module's parameters (RCCL all-reduce launched from backward hooks, averaged and sanitised per bucket) -- with one rank it only
sanitises, so the same code runs on one GPU and on N."""
import json
import os
import time

import numpy as np
import torch

from .grad_sync import BucketedAllReduce


class Phase:
    def __init__(self, name, module, opt, interval, sync=None):
        self.name, self.module, self.opt, self.interval, self.sync = name, module, opt, interval, sync
        self.start_event = self.end_event = None

    def __repr__(self):
        return f'Phase({self.name}, interval={self.interval})'


def make_phases(G, D, g_opt_kwargs, d_opt_kwargs, g_reg_interval=4, d_reg_interval=16, opt_class=torch.optim.Adam,
                process_group=None, bucket_bytes=64 << 20, timing=False):
    """[Gmain, Greg, Dmain, Dreg] (or Gboth / Dboth where the interval is None), stylegan_default.py:304-321."""
    phases = []
    for name, module, opt_kwargs, reg_interval in (('G', G, g_opt_kwargs, g_reg_interval), ('D', D, d_opt_kwargs, d_reg_interval)):
        params = [p for p in module.parameters()]
        kw = dict(opt_kwargs)
        sync = BucketedAllReduce(params, bucket_bytes=bucket_bytes, process_group=process_group) if any(p.is_cuda for p in params) or \
            torch.distributed.is_available() and torch.distributed.is_initialized() else None
        if hasattr(opt_class, 'step_from_buckets'):          # optim.ShgAdam: the step reads the gradients in the phase's buckets
            kw['sync'] = sync
        if reg_interval is None:
            opt = opt_class(params, **kw)
            sync = getattr(opt, 'sync', sync)
            phases.append(Phase(name + 'both', module, opt, 1, sync))
        else:                                   # lazy regularisation
            mb_ratio = reg_interval / (reg_interval + 1)
            kw['lr'] = kw['lr'] * mb_ratio
            kw['betas'] = tuple(float(beta) ** mb_ratio for beta in kw['betas'])
            opt = opt_class(params, **kw)
            sync = getattr(opt, 'sync', sync)              # (ShgAdam without buckets to share lays out its own)
            phases.append(Phase(name + 'main', module, opt, 1, sync))
            phases.append(Phase(name + 'reg', module, opt, reg_interval, sync))
    if timing and torch.cuda.is_available():
        for ph in phases:
            ph.start_event, ph.end_event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    return phases


_WARNED = set()


def _warn_unarmed(loss, phase):
    """The overlap of the gradient all-reduce with backward depends on the loss announcing the phase's LAST backward pass
    (``loss.grad_sync.arm()``, as StyleGAN2Loss._arm does for sync=True); a Loss that never does gets correct gradients, reduced
    bucket by bucket after backward.  Said once per loss class."""
    key = (type(loss).__name__, phase.name)
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(f'{type(loss).__name__} did not arm the gradient buckets in phase {phase.name}: the all-reduce runs after backward '
                      'instead of under it (call self.grad_sync.arm() before the last backward of a phase call with sync=True)')


def sanitize_(params):
    """``misc.nan_to_num(param.grad, nan=0, posinf=1e5, neginf=-1e5, out=param.grad)`` of stylegan_default.py:160-164."""
    for p in params:
        if p.grad is not None:
            torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5, out=p.grad)


def run_phases(real_img, z_dim, phases, batch_idx, loss, batch_gpu, effective_batch_gpu=None, device=None, real_c=None, gen_c=None):
    """One iteration = ``train_stage.main`` (stylegan_default.py:108-167).  real_img [batch_gpu, C, H, W]; returns the names of the
    phases that ran."""
    device = real_img.device if device is None else torch.device(device)
    eff = batch_gpu if effective_batch_gpu is None else effective_batch_gpu
    real_img = real_img.to(device).to(torch.float32)
    real_c = torch.zeros([batch_gpu, 0], device=device) if real_c is None else real_c.to(device)
    all_gen_c = torch.zeros([len(phases) * batch_gpu, 0], device=device) if gen_c is None else gen_c.to(device)
    all_gen_z = torch.randn([len(phases) * batch_gpu, z_dim]).to(device)       # drawn on the host like the reference (:128)
    all_gen_z, all_gen_c = all_gen_z.split(batch_gpu), all_gen_c.split(batch_gpu)
    ran = []
    for phase, phase_gen_z, phase_gen_c in zip(phases, all_gen_z, all_gen_c):
        if batch_idx % phase.interval != 0:
            continue
        if phase.start_event is not None:
            phase.start_event.record(torch.cuda.current_stream(device))
        _phase_body(phase, loss, real_img, real_c, phase_gen_z, phase_gen_c, eff)
        if phase.end_event is not None:
            phase.end_event.record(torch.cuda.current_stream(device))
        ran.append(phase.name)
    return ran


# Backward passes run on the calling thread.  With the engine's device worker thread, the nodes a create_graph backward creates
# (path-length / R1 regularisers) are numbered by that thread's counter and the forward nodes by the main thread's; the two advance by
# different amounts per iteration, so the ready-queue order of the double-backward graph -- and the order in which gradients with
# several consumers (x_global, the encoder's skip features) are summed -- changed from one execution to the next: identical inputs
# gave parameters that differed in the last bits (tools/ARCHIVE.md: probes/autograd_thread_order.py; every kernel is bit-repeatable).  One
# GPU per process means the worker thread bought no concurrency anyway.
SINGLE_THREADED_BACKWARD = os.environ.get('SHG_ENGINE_THREADS', '0') != '1'


def _phase_backward(phase, loss, real_img, real_c, gen_z, gen_c, eff):
    """First half of a phase (stylegan_default.py:141-158): zero the gradients, open the phase's module, run the loss's forward and
    backward passes over the rounds.  Bucket all-reduces are launched from the backward hooks (eager loop) unless ``phase.sync.defer``."""
    if phase.sync is not None:
        phase.sync.zero_grad()                       # gradients live in the all-reduce buckets
    else:
        phase.opt.zero_grad(set_to_none=True)
    phase.module.requires_grad_(True)
    if hasattr(loss, 'grad_sync'):
        loss.grad_sync = phase.sync                  # the loss arms it before the phase's LAST backward (sync=True round only)
    rr, rc, gz, gc = real_img.split(eff), real_c.split(eff), gen_z.split(eff), gen_c.split(eff)
    with torch.autograd.set_multithreading_enabled(not SINGLE_THREADED_BACKWARD):
        for round_idx in range(len(rr)):
            loss.accumulate_gradients(phase=phase.name, real_img=rr[round_idx], real_c=rc[round_idx], gen_z=gz[round_idx],
                                      gen_c=gc[round_idx], sync=(round_idx == len(rr) - 1), gain=phase.interval)
    phase.module.requires_grad_(False)
    if hasattr(loss, 'grad_sync'):
        loss.grad_sync = None


def _phase_step(phase, loss=None, reduced=False):
    """Second half (stylegan_default.py:159-166): gradients averaged over the ranks and sanitised, optimiser step.  ``reduced``: the
    buckets were all-reduced by ``phase.sync.reduce_all()`` already (split-graph form)."""
    if phase.sync is not None:
        if phase.sync.reduce and not reduced and not phase.sync.was_armed():
            _warn_unarmed(loss, phase)               # correct, but every bucket is reduced synchronously in finish(): no overlap
        if hasattr(phase.opt, 'step_from_buckets'):  # optim.ShgAdam: average, sanitise and step in one pass over the buckets
            phase.opt.step_from_buckets(reduced=reduced)
            return
        phase.sync.finish(reduced=reduced)           # waits for the bucket all-reduces, averages, nan_to_num
        for p in phase.sync.untouched():             # as after zero_grad(set_to_none=True): the optimiser skips them
            p.grad = None
    else:
        sanitize_(phase.module.parameters())
    phase.opt.step()


def _phase_body(phase, loss, real_img, real_c, gen_z, gen_c, eff):
    """One phase of an iteration on given tensors: the inner block of ``run_phases`` (stylegan_default.py:141-166)."""
    _phase_backward(phase, loss, real_img, real_c, gen_z, gen_c, eff)
    _phase_step(phase, loss)


class PhaseGraphs:
    """``run_phases`` with every phase captured ONCE as a HIP graph and replayed afterwards.

    A G + D step of the FFHQ-512 networks is ~4 500 kernel launches (convolutions forward / backward / weight gradient, FIR, layer
    tails, ~2 000 small elementwise kernels of autograd glue and the optimiser); the Python + autograd + ctypes path needs ~85 ms
    to enqueue them, about what the GPU needs to run them -- the step is host-bound as soon as the kernels get faster.  A phase
    has static shapes and no host read on the device path (style-mixing cutoff, lazy-regulariser means and the Adam step counter
    live on the device: ``Adam(capturable=True)`` is required), so ``torch.cuda.graph`` can record zero_grad -> forward(s) ->
    backward(s) -> gradient sanitisation -> optimiser step as one graph per phase.  Replays read the real batch and the latents
    from static buffers that ``run`` fills first.

    Parameter-derived caches (prepared weight layouts of no-grad passes) are keyed on version counters, which a replay does not
    advance: the caches are invalidated around captures and after every replay.

    More than one rank (an active ``BucketedAllReduce``): a phase is TWO graphs with the collective between them on the host side --
    graph A = zero_grad -> forward(s) -> backward(s) into the buckets (hooks deferred: no collective is captured), then
    ``sync.reduce_all()`` (every bucket in flight at once over RCCL), then graph B = average + sanitise + optimiser step.  What is given
    up against the eager loop is the overlap of the reduction with backward (G: 5 buckets of 64 MiB, D: 4; about 2 ms of ring
    all-reduce per phase on xGMI), what is gained is the host enqueue of ~2 000 launches per phase; ``bench.py`` times both forms and
    takes the faster one on all ranks together."""

    def __init__(self, phases, loss, batch_gpu, z_dim, real_shape, device, effective_batch_gpu=None, warmup=2):
        self.phases, self.loss, self.b, self.z_dim = phases, loss, batch_gpu, z_dim
        self.device = torch.device(device)
        self.eff = batch_gpu if effective_batch_gpu is None else effective_batch_gpu
        self.real = torch.zeros(real_shape, device=self.device, dtype=torch.float32)
        self.real_c = torch.zeros([batch_gpu, 0], device=self.device)
        self.gen_c = torch.zeros([batch_gpu, 0], device=self.device)
        self.z = {ph.name: torch.zeros([batch_gpu, z_dim], device=self.device) for ph in phases}
        self.graphs = {}
        self.seen = {ph.name: 0 for ph in phases}
        self.warmup = warmup
        if warmup < 1:
            raise ValueError('PhaseGraphs: warmup >= 1 (lazily built constants, Adam state and allocator pools must exist before the capture)')
        # more than one rank: two graphs per phase.  Decided per phase (a phase without a reducing sync is one graph, whatever the others
        # are); ``split`` says whether any phase takes the two-graph form
        self.split_of = {ph.name: ph.sync is not None and bool(ph.sync.reduce) for ph in phases}
        self.split = any(self.split_of.values())
        for ph in phases:
            if hasattr(ph.opt, 'step_from_buckets'):       # optim.ShgAdam keeps its step counters on the device by construction
                continue
            for g in ph.opt.param_groups:
                if not g.get('capturable', False):
                    raise ValueError('PhaseGraphs: build the optimisers with capturable=True (the step counter must live on the device)')

    def _invalidate(self):
        from .model_zoo.stylegan import _ParamCache
        _ParamCache.invalidate_all()

    def run(self, real_img, batch_idx):
        """One iteration; the first ``warmup`` runs of a phase are eager (allocator, lazily built constants), the next one is
        captured.  Returns the names of the phases that ran."""
        all_z = torch.randn([len(self.phases) * self.b, self.z_dim]).to(self.device)      # drawn on the host like the reference (:128)
        self.real.copy_(real_img.to(self.device, torch.float32))
        ran = []
        for ph, z in zip(self.phases, all_z.split(self.b)):
            if batch_idx % ph.interval != 0:
                continue
            self.z[ph.name].copy_(z)
            g = self.graphs.get(ph.name)
            split = self.split_of[ph.name]
            if ph.start_event is not None:                   # (around the replay, not inside the graph)
                ph.start_event.record(torch.cuda.current_stream(self.device))
            if g is None and self.seen[ph.name] < self.warmup:
                self.seen[ph.name] += 1
                _phase_body(ph, self.loss, self.real, self.real_c, self.z[ph.name], self.gen_c, self.eff)
            else:
                if g is None and not split:
                    self._invalidate()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        _phase_body(ph, self.loss, self.real, self.real_c, self.z[ph.name], self.gen_c, self.eff)
                    self.graphs[ph.name] = g
                elif g is None:
                    # two graphs around the host-side collective.  Nothing is reduced while capturing; whether the capture worked is agreed
                    # between the ranks BEFORE the first collective of the replay (a rank that failed alone would leave the others
                    # waiting in reduce_all): all ranks raise together and the caller falls back to run_phases together.
                    self._invalidate()
                    ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                    err = None
                    ph.sync.defer = True
                    try:
                        with torch.cuda.graph(ga):
                            _phase_backward(ph, self.loss, self.real, self.real_c, self.z[ph.name], self.gen_c, self.eff)
                        ph.sync.defer = False
                        with torch.cuda.graph(gb, pool=ga.pool()):
                            _phase_step(ph, self.loss, reduced=True)
                    except Exception as e:              # noqa: BLE001 -- reported below, on every rank
                        err = e
                    finally:
                        ph.sync.defer = False
                    ok = torch.tensor([0.0 if err is not None else 1.0], device=self.device if torch.distributed.get_backend(ph.sync.group) == 'nccl' else 'cpu')
                    torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN, group=ph.sync.group)
                    if float(ok.item()) < 1.0:
                        raise RuntimeError(f'PhaseGraphs: capture of phase {ph.name} failed on ' + ('this rank: ' + repr(err) if err is not None else 'another rank'))
                    g = self.graphs[ph.name] = (ga, gb)
                if split:
                    g[0].replay()
                    ph.sync.reduce_all()
                    g[1].replay()
                else:
                    g.replay()
                self._invalidate()
            if ph.end_event is not None:
                ph.end_event.record(torch.cuda.current_stream(self.device))
            ran.append(ph.name)
        return ran


def ema_beta(batch_size, cur_nimg, ema_kimg=10.0, ema_rampup=None):
    ema_nimg = ema_kimg * 1000
    if ema_rampup is not None:
        ema_nimg = min(ema_nimg, cur_nimg * ema_rampup)
    return 0.5 ** (batch_size / max(ema_nimg, 1e-8))


@torch.no_grad()
def update_ema(G_ema, G, batch_size, cur_nimg, ema_kimg=10.0, ema_rampup=None):
    """stylegan_default.py:383-390."""
    beta = ema_beta(batch_size, cur_nimg, ema_kimg, ema_rampup)
    for p_ema, p in zip(G_ema.parameters(), G.parameters()):
        p_ema.copy_(p.lerp(p_ema, beta))
    for b_ema, b in zip(G_ema.buffers(), G.buffers()):
        b_ema.copy_(b)
    return beta


# ---- what a run keeps: sample grids, snapshots, the tick block (stylegan_default.py:402-575) ---------------------------------------------
SNAPSHOT_VERSION = 1


def _rank_world():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1


def image_grid(images, grid_size, drange=(-1, 1), real=None, mask=None):
    """``draw_functor.output`` (stylegan_default.py:74-84) on the device: float32 [gw * gh, C, H, W] (C 1 or 3) -> uint8
    [gh * H, gw * W, C], ``(uint8) clip(rint((x - lo) * (255 / (hi - lo))), 0, 255)`` in float32 with numpy's rounding (ties to even).
    ``real`` / ``mask`` ([N, C, H, W] / [N, 1, H, W]): the grid of ``real * mask + images * (1 - mask)`` (shgan_default.py:107)."""
    import ctypes
    from . import _lib, kernels
    gw, gh = (int(v) for v in grid_size)
    lo, hi = (float(v) for v in drange)
    if not hi > lo:
        raise ValueError(f'image_grid: drange must be (lo, hi) with hi > lo (got {drange})')
    if not isinstance(images, torch.Tensor) or images.ndim != 4 or images.shape[1] not in (1, 3):
        raise ValueError('image_grid: float32 [N, C, H, W] with C 1 or 3 expected')
    n, c, h, w = images.shape
    if gw < 1 or gh < 1 or n != gw * gh:
        raise ValueError(f'image_grid: {n} images do not fill a {gw} x {gh} grid')
    if (real is None) != (mask is None):
        raise ValueError('image_grid: real and mask go together')
    if real is not None and (real.shape != images.shape or mask.shape != (n, 1, h, w)):
        raise ValueError('image_grid: real like the images and mask [N, 1, H, W] expected')
    launch = kernels._Launch()               # (``launch``, not ``L``: the allocation tests cover this function from tests/test_gpu_train_run.py)
    images = launch.req(images, 'images')
    real, mask = launch.req(real, 'real'), launch.req(mask, 'mask')
    out = launch.new([gh * h, gw * w, c], torch.uint8)           # every byte is written
    scale = float(np.float32(255.0 / (hi - lo)))
    with launch:
        _lib.check(_lib.get_lib().shg_image_grid_u8(
            ctypes.c_void_p(images.data_ptr()), ctypes.c_void_p(real.data_ptr() if real is not None else None),
            ctypes.c_void_p(mask.data_ptr() if mask is not None else None), ctypes.c_void_p(out.data_ptr()), c, h, w, gw, gh, lo, scale,
            launch.stream()), 'image_grid_u8')
    return out


def save_image_grid(u8, path):
    """uint8 [H, W, 1 or 3] (device or host) -> a PNG, written atomically (Pillow on the host)."""
    import PIL.Image
    arr = u8.cpu().numpy() if isinstance(u8, torch.Tensor) else np.asarray(u8)
    img = PIL.Image.fromarray(arr[:, :, 0], 'L') if arr.shape[2] == 1 else PIL.Image.fromarray(arr, 'RGB')
    atomic_write(path, lambda tmp: img.save(tmp, format='PNG'))


def atomic_write(path, write_fn):
    """``write_fn(tmp)`` writes a temporary file in ``path``'s directory, which then takes ``path``'s place in one step (``os.replace``);
    a writer that raises leaves what was at ``path`` as it was and no temporary file behind."""
    path = os.fspath(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f'{path}.tmp{os.getpid()}'
    try:
        write_fn(tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _distinct_opts(phases):
    """[(key, optimiser)], one entry per optimiser object: the phases that share one ('Gmain' / 'Greg') give the key 'Gmain+Greg'."""
    out = []
    for ph in phases or ():
        hit = [e for e in out if e[1] is ph.opt]
        if hit:
            hit[0][0].append(ph.name)
        else:
            out.append(([ph.name], ph.opt))
    return [('+'.join(names), opt) for names, opt in out]


def health_prefixes(phases):
    """[(prefix, optimiser)] for the optimisers built with ``health=True``: the stem its phase names share once 'main' / 'reg' / 'both' is
    taken off ('Gmain+Greg' -> 'G'); an optimiser whose phases share no such stem, or whose stem another optimiser has too, keeps its whole
    key ('Gmain+Greg'), so that two optimisers never fold into one ``Grad/<prefix>/*`` slot."""
    stems = []
    for key, opt in _distinct_opts(phases):
        if not getattr(opt, 'health', False):
            continue
        found = set()
        for name in key.split('+'):
            hit = [name[:-len(sfx)] for sfx in ('main', 'reg', 'both') if name.endswith(sfx) and len(name) > len(sfx)]
            found.add(hit[0] if hit else None)
        stems.append((found.pop() if len(found) == 1 else None, key, opt))
    count = {}
    for stem, _, _ in stems:
        count[stem] = count.get(stem, 0) + 1
    return [(stem if stem is not None and count[stem] == 1 else key, opt) for stem, key, opt in stems]


def jsonl_fields(stats):
    """``Collector.as_dict()`` as one ``stats.jsonl`` line holds it: a name that received nothing in the tick is left out (the reference's
    line holds the reported names only), and a value that is not finite is written as null -- the line is strict JSON."""
    out = {}
    for name, d in stats.items():
        if d['num'] == 0 and not d.get('nonfinite'):
            continue
        out[name] = {k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in d.items()}
    return out


def _rng_state(device):
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    st = {'torch': torch.get_rng_state(), 'numpy': {'kind': str(kind), 'keys': torch.from_numpy(np.asarray(keys, np.int64).copy()), 'pos': int(pos),
                                                    'has_gauss': int(has_gauss), 'cached_gaussian': float(cached)}}
    if device is not None and torch.device(device).type == 'cuda':
        st['cuda'] = torch.cuda.get_rng_state(device)
    return st


def _set_rng_state(st, device):
    torch.set_rng_state(st['torch'].cpu())
    n = st['numpy']
    np.random.set_state((n['kind'], n['keys'].cpu().numpy().astype(np.uint32), n['pos'], n['has_gauss'], n['cached_gaussian']))
    if 'cuda' in st and device is not None and torch.device(device).type == 'cuda':
        torch.cuda.set_rng_state(st['cuda'].cpu(), device)


def save_snapshot(path, G, D, G_ema, phases=None, loss=None, ada=None, progress=None, device=None, save_fn=None):
    """One ``torch.save``d dict of state_dicts (no pickled modules): the three networks, one entry per DISTINCT optimiser of ``phases``,
    the loss state (``pl_mean``), the loss's augment pipe and ``ada`` (an ``AdaController``), ``progress`` (``cur_nimg``, ``batch_idx``,
    ``cur_tick``, ``tick_start_nimg``), the RNG states of every rank (host, device, numpy; gathered to rank 0) and the format version and
    world size.  Rank 0 writes, atomically; beside it ``G_ema-<kimg:06d>.pth``, the bare ``G_ema.state_dict()``.  A collective when
    ``torch.distributed`` is initialised: every rank calls it.  Returns the dict on rank 0, None elsewhere."""
    rank, world = _rank_world()
    rng = _rng_state(device)
    if world > 1:
        gathered = [None] * world if rank == 0 else None
        torch.distributed.gather_object(rng, gathered, dst=0)
    else:
        gathered = [rng]
    if rank != 0:
        return None
    progress = dict(progress or {})
    for k in ('cur_nimg', 'batch_idx', 'cur_tick', 'tick_start_nimg'):
        progress[k] = int(progress.get(k, 0))
    pipe = getattr(loss, 'augment_pipe', None)
    snap = {
        'version': SNAPSHOT_VERSION, 'world': world, 'progress': progress,
        'G': G.state_dict(), 'D': D.state_dict(), 'G_ema': G_ema.state_dict(),
        'opt': {key: opt.state_dict() for key, opt in _distinct_opts(phases)},
        'loss': loss.state_dict() if hasattr(loss, 'state_dict') else {},
        'augment_pipe': pipe.state_dict() if pipe is not None else None,
        'ada': ada.state_dict() if ada is not None else None,
        'rng': gathered,
    }
    save = torch.save if save_fn is None else save_fn
    atomic_write(path, lambda tmp: save(snap, tmp))
    ema_path = os.path.join(os.path.dirname(os.path.abspath(path)), 'G_ema-%06d.pth' % (progress['cur_nimg'] // 1000))
    atomic_write(ema_path, lambda tmp: save(snap['G_ema'], tmp))
    return snap


def load_snapshot(path, G, D, G_ema, phases=None, loss=None, ada=None, device=None):
    """Restore what ``save_snapshot`` wrote, on every rank (rank r takes RNG entry r).  Raises on another format version or world size,
    naming both.  Returns the progress dict."""
    rank, world = _rank_world()
    snap = torch.load(path, map_location='cpu', weights_only=True)
    if snap.get('version') != SNAPSHOT_VERSION:
        raise RuntimeError(f'load_snapshot: {path} has format version {snap.get("version")}, this code reads version {SNAPSHOT_VERSION}')
    if snap.get('world') != world:
        raise RuntimeError(f'load_snapshot: {path} was written by {snap.get("world")} ranks, this run has {world} '
                           '(resuming with another world size is not supported)')
    G.load_state_dict(snap['G'])
    D.load_state_dict(snap['D'])
    G_ema.load_state_dict(snap['G_ema'])
    opts = _distinct_opts(phases)
    if sorted(snap['opt']) != sorted(k for k, _ in opts):
        raise RuntimeError(f'load_snapshot: {path} holds the optimisers {sorted(snap["opt"])}, the phases have {sorted(k for k, _ in opts)}')
    for key, opt in opts:
        opt.load_state_dict(snap['opt'][key])
    if hasattr(loss, 'load_state_dict') and snap['loss']:
        loss.load_state_dict(snap['loss'])
    pipe = getattr(loss, 'augment_pipe', None)
    if (pipe is None) != (snap['augment_pipe'] is None) or (ada is None) != (snap['ada'] is None):
        raise RuntimeError(f'load_snapshot: {path} and this run differ in whether there is an augment pipe / an ADA controller')
    if pipe is not None:
        pipe.load_state_dict(snap['augment_pipe'])
    if ada is not None:
        ada.load_state_dict(snap['ada'])
    _set_rng_state(snap['rng'][rank], device)
    return dict(snap['progress'])


class Maintenance:
    """The tick block of stylegan_default.py:402-575 for ``train``: conditions (``done or cur_tick % k == 0``; None = never) and order of the
    reference -- status line, metrics, image, snapshot, statistics.
    ``metrics``: {name: callable(G_ema) -> {key: float}}, reported as ``Metrics/<key>``.
    ``grid``: (inputs, (gw, gh)); inputs = {'batches': [kwargs of a G_ema call, ...], 'real': [N, 3, H, W] or None, 'mask': [N, 1, H, W] or
    None}: ``fakes<kimg>.png`` from the concatenated outputs and, with real and mask, ``fakes<kimg>_combined.png``.
    Files under ``log_dir``: ``stats.jsonl`` (one line per tick, appended), ``fakes*.png``, ``weight/network-snapshot-<kimg>.pt`` and
    ``weight/G_ema-<kimg>.pth``.  Rank 0 writes; the collectives (collector all-reduce, RNG gather) run on every rank."""

    def __init__(self, log_dir, snapshot_ticks=None, image_ticks=None, metric_ticks=None, metrics=None, grid=None, drange=(-1, 1),
                 print_fn=print):
        self.log_dir = os.fspath(log_dir)
        self.snapshot_ticks, self.image_ticks, self.metric_ticks = snapshot_ticks, image_ticks, metric_ticks
        self.metrics = dict(metrics or {})
        self.grid, self.drange, self.print_fn = grid, drange, print_fn
        self.start_time = self.tick_start_time = time.time()
        self.maintenance_time = 0.0
        self.snapshots, self.images, self.lines = [], [], []          # what this object wrote / logged (paths, paths, dicts)

    @staticmethod
    def due(ticks, cur_tick, done):
        return ticks is not None and (done or cur_tick % ticks == 0)

    def snapshot_path(self, cur_nimg):
        return os.path.join(self.log_dir, 'weight', 'network-snapshot-%06d.pt' % (cur_nimg // 1000))

    @torch.no_grad()
    def draw_grid(self, G_ema, cur_nimg):
        inputs, grid_size = self.grid
        was_training = G_ema.training
        G_ema.eval()
        try:
            images = torch.cat([G_ema(**kw).to(torch.float32) for kw in inputs['batches']])
        finally:
            G_ema.train(was_training)
        out = [os.path.join(self.log_dir, 'fakes%06d.png' % (cur_nimg // 1000))]
        grids = [image_grid(images, grid_size, self.drange)]
        if inputs.get('real') is not None and inputs.get('mask') is not None:
            out.append(os.path.join(self.log_dir, 'fakes%06d_combined.png' % (cur_nimg // 1000)))
            grids.append(image_grid(images, grid_size, self.drange, real=inputs['real'], mask=inputs['mask']))
        if _rank_world()[0] == 0:
            for path, u8 in zip(out, grids):
                save_image_grid(u8, path)
                self.images.append(path)

    def tick(self, collector, cur_tick, cur_nimg, batch_idx, tick_start_nimg, done, G, D, G_ema, phases, loss, ada, device):
        """One tick; ``progress`` in a snapshot is the state the NEXT iteration starts from (``cur_tick + 1``, tick start = ``cur_nimg``)."""
        rank = _rank_world()[0]
        now = time.time()
        pipe = getattr(loss, 'augment_pipe', None)
        r0 = collector.report0
        fields = [f"tick {r0('Progress/tick', cur_tick):<5d}", f"kimg {r0('Progress/kimg', cur_nimg / 1e3):<8.1f}",
                  f"time {r0('Timing/total_sec', now - self.start_time):<10.1f}",
                  f"sec/tick {r0('Timing/sec_per_tick', now - self.tick_start_time):<7.1f}",
                  f"sec/kimg {r0('Timing/sec_per_kimg', (now - self.tick_start_time) / max(cur_nimg - tick_start_nimg, 1) * 1e3):<7.2f}",
                  f"maintenance {r0('Timing/maintenance_sec', self.maintenance_time):<6.1f}",
                  f"augment {r0('Progress/augment', float(pipe.p.cpu()) if pipe is not None else 0.0):.3f}"]
        if rank == 0 and self.print_fn is not None:
            self.print_fn(' '.join(fields))
        if self.metrics and self.due(self.metric_ticks, cur_tick, done):
            for name, fn in self.metrics.items():
                for key, value in fn(G_ema).items():
                    r0(f'Metrics/{key}', float(value))
        if self.grid is not None and self.due(self.image_ticks, cur_tick, done):
            self.draw_grid(G_ema, cur_nimg)
        if self.due(self.snapshot_ticks, cur_tick, done):
            path = self.snapshot_path(cur_nimg)
            save_snapshot(path, G, D, G_ema, phases=phases, loss=loss, ada=ada, device=device,
                          progress=dict(cur_nimg=cur_nimg, batch_idx=batch_idx, cur_tick=cur_tick + 1, tick_start_nimg=cur_nimg))
            if rank == 0:
                self.snapshots.append(path)
        for ph in phases:                                # per-phase milliseconds of the last run of the phase (make_phases(timing=True))
            if ph.start_event is not None and ph.end_event is not None:
                try:
                    ph.end_event.synchronize()
                    r0('Timing/' + ph.name, ph.start_event.elapsed_time(ph.end_event))
                except RuntimeError:                     # an event that was never recorded (a phase that has not run since the resume)
                    pass
        for prefix, opt in health_prefixes(phases):
            opt.health_report(collector, prefix)
        collector.update()
        line = dict(jsonl_fields(collector.as_dict()), timestamp=time.time())
        self.lines.append(line)
        if rank == 0:
            os.makedirs(self.log_dir, exist_ok=True)
            with open(os.path.join(self.log_dir, 'stats.jsonl'), 'at') as fh:
                fh.write(json.dumps(line, allow_nan=False) + '\n')
        self.tick_start_time = time.time()
        self.maintenance_time = self.tick_start_time - now
        return line


def train(G, D, G_ema, loss, batches, phases, z_dim, batch_size, batch_gpu, total_kimg, effective_batch_gpu=None, ema_kimg=10.0,
          ema_rampup=None, kimg_per_tick=4, on_tick=None, device=None, ema=None, ada=None, graphs=None, collector=None, maintenance=None,
          resume=None):
    """The iteration loop of stylegan_default.py:370-396: ``batches`` yields real images [batch_gpu, C, H, W] for this rank,
    ``batch_size`` is the GLOBAL batch (= batch_gpu * world).  ``ema``: an ``optim.EmaUpdater(G_ema, G)`` (one launch per iteration)
    in place of ``update_ema``.  ``ada``: an ``ada.AdaController`` over the loss's augment pipe, fed the signs of the real logits after the
    EMA update (stylegan_default.py:397-400).  Returns (cur_nimg, batch_idx).

    The run around it, all optional: ``graphs``: a ``PhaseGraphs`` over the same phases and loss, used instead of ``run_phases``.
    ``maintenance``: a ``Maintenance`` -- the tick block (:402-575); its statistics go through ``collector`` (a
    ``training_stats.Collector``, the one the loss and ``health_report`` feed; one is made when none is given).  ``resume``: the path of a
    ``save_snapshot`` file, restored before the first iteration -- networks, optimisers, loss, ADA, counters and RNG states; ``batches`` may
    then be a callable ``batch_idx -> iterator`` so that the data stream is re-entered where it stood (an iterator is taken as it is)."""
    cur_nimg, batch_idx, cur_tick, tick_start = 0, 0, 0, 0
    if resume is not None:
        prog = load_snapshot(resume, G, D, G_ema, phases=phases, loss=loss, ada=ada, device=device)
        cur_nimg, batch_idx, cur_tick, tick_start = prog['cur_nimg'], prog['batch_idx'], prog['cur_tick'], prog['tick_start_nimg']
        if cur_nimg >= total_kimg * 1000:
            return cur_nimg, batch_idx
    if maintenance is not None and collector is None:
        from .training_stats import Collector
        collector = Collector(device if device is not None else next(G.parameters()).device)
    if callable(batches):
        batches = batches(batch_idx)
    for real_img in batches:
        if graphs is not None:
            graphs.run(real_img, batch_idx)
        else:
            run_phases(real_img, z_dim, phases, batch_idx, loss, batch_gpu, effective_batch_gpu, device)
        if ema is not None:
            ema.update(batch_size, cur_nimg, ema_kimg, ema_rampup)
        else:
            update_ema(G_ema, G, batch_size, cur_nimg, ema_kimg, ema_rampup)
        if ada is not None and 'Loss/signs/real' in getattr(loss, 'stats', {}):
            ada.update(loss.stats['Loss/signs/real'], batch_size)
        cur_nimg += batch_size
        batch_idx += 1
        done = cur_nimg >= total_kimg * 1000
        if done or cur_tick == 0 or cur_nimg >= tick_start + kimg_per_tick * 1000:
            if maintenance is not None:
                maintenance.tick(collector, cur_tick, cur_nimg, batch_idx, tick_start, done, G, D, G_ema, phases, loss, ada, device)
            if on_tick is not None:
                on_tick(cur_tick, cur_nimg, batch_idx)
            cur_tick += 1
            tick_start = cur_nimg
        if done:
            break
    return cur_nimg, batch_idx
