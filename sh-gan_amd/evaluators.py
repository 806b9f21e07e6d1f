"""The evaluators of ``eval_harness.EvalLoop`` and their two helpers.  An evaluator owns one option group: its checks, buffers, ``add(out,
real, k0)`` on the batch's stream (``out``: uint8 composite of this rank's items k0 .. k0+B-1), ``finish(collect)`` from ``gather`` and value."""
import torch

from .fid_stats import FidStats, fid_from_stats, frechet_device
from .ids_score import ids_from_features
from .image_metrics import MetricsAccumulator, finish_metrics
from .inception_score import is_accumulate, is_from_accumulator, new_accumulator, split_of
from .kid import kid_from_features
from .precision_recall import pr_from_features


def zipzap_device(full, n_items):
    """``zipzap_arrange`` (eva_base.py:196-230) of equally long rank shards, on the device: full [world, n_local, ...] (rank r's
    k-th result at [r, k]) -> [n_items, ...] in dataset order (item k*world + r), the padded duplicates of
    ``DistributedSampler(extend=True)`` cut off.  One transposing copy instead of a host round trip of the whole result set."""
    world, n_local = full.shape[:2]
    return full.transpose(0, 1).reshape((world * n_local,) + tuple(full.shape[2:]))[:n_items]


class Collective:
    """The end-of-run collectives over the ranks' shards of ``n_items`` items: RCCL over xGMI on GPUs, gloo for the CPU tests.  Without a
    process group every method is the 1-rank identity; a 1-rank group goes through the collective (the path of N ranks)."""

    def __init__(self, device, n_items, world):
        import torch.distributed as dist
        self.device, self.n_items, self.world = torch.device(device), int(n_items), int(world)
        self.dist = dist if dist.is_available() and dist.is_initialized() else None
        # RCCL takes device tensors; a gloo group (CPU tests, ranks sharing one device) is handed host tensors
        self.via_host = self.dist is not None and self.dist.get_backend() == 'gloo' and self.device.type == 'cuda'

    def rows(self, local, arrange=True):
        """This rank's [n_local, ...] (any dtype) -> [n_items, ...] in dataset order on the device: one ``all_gather_into_tensor`` and
        ``zipzap_device``.  ``arrange=False`` stops at [world, n_local, ...], for finish_metrics alone, which re-interleaves per column."""
        full = local[None]
        if self.dist is not None:
            src = local.cpu() if self.via_host else local
            full = torch.empty((self.world,) + tuple(src.shape), dtype=src.dtype, device=src.device)
            self.dist.all_gather_into_tensor(full.view((-1,) + tuple(src.shape[1:])), src)
        return zipzap_device(full.to(self.device), self.n_items) if arrange else full.to(self.device)

    def sum_(self, t):
        """``t`` summed over the ranks, in place: one ``all_reduce``."""
        if self.dist is not None:
            h = t.cpu() if self.via_host else t
            self.dist.all_reduce(h, op=self.dist.ReduceOp.SUM)
            t.copy_(h)                      # (nothing to copy when h is t)


class PerStream:
    """One accumulator per stream: a kernel that accumulates in place must not share its target with a batch on another stream.  ``prepare``
    creates one ``factory()`` per stream key up front (``None``: the caller's stream; ``factory=None``, an option that is off: nothing);
    ``here()`` is the current stream's, else the caller's; ``total()`` adds them up once into ``sum`` (None if none) and drops the parts."""

    def __init__(self, factory, device, add=lambda into, part: into.add_(part)):
        self.factory, self.device, self.add, self.parts, self.sum = factory, torch.device(device), add, {}, None

    def prepare(self, stream_keys):
        for key in stream_keys:
            if self.factory is not None and key not in self.parts:
                self.parts[key] = self.factory()

    def here(self):
        cur = torch.cuda.current_stream(self.device).cuda_stream if self.device.type == 'cuda' else None
        self.prepare([None])                # (only a caller that never ran prepare() gets the caller's stream's created here)
        return self.parts.get(cur, self.parts[None])

    def total(self):
        parts, self.parts = list(self.parts.values()), {}
        if self.sum is None and parts:
            self.sum = parts.pop(0)
        for p in parts:
            self.add(self.sum, p)
        return self.sum


def check_fid_tail(fid_tail):
    """'host' | 'device' | dict(tol=, max_iter=, matmul_fn=) (= 'device' with options) -> (mode, options); anything else is a ValueError."""
    if isinstance(fid_tail, dict):
        unknown = set(fid_tail) - {'tol', 'max_iter', 'matmul_fn'}
        if unknown:
            raise ValueError(f'EvalLoop: unknown fid_tail option(s) {sorted(unknown)}')
        return 'device', dict(fid_tail)
    if fid_tail not in ('host', 'device'):
        raise ValueError(f"EvalLoop: fid_tail must be 'host' or 'device' (or a dict of frechet_device options), got {fid_tail!r}")
    return fid_tail, {}


class DetectorStats:
    """Everything that hangs off ``feature_fn``, the detector hand-off of eva_fid.py:194-206 (``shard``: the EvalLoop), one detector run per side per
    batch.  Per batch ``feature_fn(images)`` -> fp64 moments on the device (fid_stats.FidStats; padded duplicates weigh 0).  The moment kernel
    accumulates in place, so every stream owns a partial accumulator; ``finish`` adds them up and all-reduces the sum once (``fake.sum``).
    ``fid_real=True`` adds the real side (eva_fid.py's ``compute_fid`` without its cache file): ``feature_fn(real, input_range='pm1')`` (the detector
    maps [-1, 1] floats, or a loader's decoded uint8 pixels, as the reference's ``real*127.5 + 127.5``) into moments of its own (``real.sum``);
    ``fid_value()`` is ``fid_from_stats`` on both ``mean_cov``. ``kid=True`` or ``kid=dict(num_subsets=100, max_subset_size=1000, seed=0)`` adds the
    Kernel Inception Distance (stylegan_metrics/ kernel_inception_distance.py; needs ``fid_real=True``): the feature rows also go into two per-rank
    float32 buffers ``[n_local, fid_dim]`` at the batch's shard position; ``finish_kid`` gathers them to exactly ``n_items`` rows per side in dataset
    order (``kid_features``) and ``kid_value()`` runs kid.kid_from_features on them (``sums_fn`` in the dict replaces the kernel: CPU tests).
    ``inception_score=dict(num_splits=10)`` adds the Inception Score of the fakes (stylegan_metrics/inception_score.py): the batch's one run of the
    trunk becomes ``feature_fn(images, with_probs=True) -> (features, probabilities)`` and the probabilities go into a per-stream float64
    ``[num_splits, C + 2]`` accumulator (inception_score.py here; an image's split follows its dataset position, padded duplicates are skipped).
    ``C`` is ``feature_fn.num_classes`` or the dict's ``num_classes``; ``no_output_bias`` (default True, as the reference) is passed on when given;
    ``accumulate_fn(acc, probs, splits)`` replaces the kernel (CPU tests).  ``finish_is`` all-reduces the streams' sum once (``is_parts.sum``);
    ``is_value()`` -> (mean, std) over the splits.  ``pids_uids=True`` or ``pids_uids=dict(C=1.0, tol=1e-9, max_newton=100)`` adds CoModGAN's
    inception discriminative scores (ids_score.py; needs ``fid_real=True``: fake i is the completion of real i).  It keeps the feature rows in the
    two per-rank buffers KID keeps -- one pair of buffers and one pair of all-gathers (``finish_kid``) whether one or both options are on, so
    ``kid_features`` is set by either, while ``kid_value()`` stays None without ``kid`` -- and ``ids_value()`` -> (U-IDS, P-IDS) fits the linear
    SVM on this device from the gathered rows (like ``pr_value()``, not sharded over the ranks; ``pass_fn`` in the dict replaces the kernel: CPU
    tests).  ``fid_tail='device'`` (default 'host': ``fid_from_stats``, scipy's ``sqrtm`` on the host) makes ``fid_value()`` the ``fid`` of
    fid_stats.frechet_device on both ``mean_cov_device`` -- the moments never leave the device, the trace of the matrix square root comes from
    Newton-Schulz products on the fp64-MFMA GEMM -- and keeps that call's dict (trace, step count, stop reason) as ``fid_tail_info``;
    ``fid_tail=dict(tol=1e-10, max_iter=100)`` is 'device' with those options (``matmul_fn`` in the dict replaces the kernel: CPU tests).  Like
    ``pr_value()`` it runs on the caller's rank from the reduced moments.  A ``*_value()`` is None until its option is on and finished."""

    def __init__(self, shard, feature_fn, fid_dim=2048, accumulate_fn=None, fid_real=False, kid=None, inception_score=None, pids_uids=None,
                 fid_tail='host'):
        if fid_real and feature_fn is None:
            raise ValueError('EvalLoop: fid_real needs a feature_fn (the detector)')
        self.fid_tail, self.fid_tail_opts, self.fid_tail_info = check_fid_tail(fid_tail) + (None,)
        self.shard, self.feature_fn, self.needs_real, n_local = shard, feature_fn, bool(fid_real), len(shard.ids)
        self.fake, self.real = (PerStream((lambda: FidStats(fid_dim, device=shard.device, accumulate_fn=accumulate_fn)) if on else None,
                                          shard.device, add=lambda into, part: into.S.add_(part.S)) for on in (True, fid_real))
        self.kid_opts = self.kid_local = self.kid_features = self.is_opts = self.is_splits = self.ids_opts = None
        if kid:
            if feature_fn is None or not fid_real:
                raise ValueError('EvalLoop: kid needs a feature_fn (the detector) and fid_real=True (the real side\'s features)')
            self.kid_opts = dict(kid) if isinstance(kid, dict) else {}
            unknown = set(self.kid_opts) - {'num_subsets', 'max_subset_size', 'seed', 'sums_fn'}
            if unknown:
                raise ValueError(f'EvalLoop: unknown kid option(s) {sorted(unknown)}')
        if pids_uids:
            if feature_fn is None or not fid_real:
                raise ValueError('EvalLoop: pids_uids needs a feature_fn (the detector) and fid_real=True (the real side\'s features)')
            self.ids_opts = dict(pids_uids) if isinstance(pids_uids, dict) else {}
            unknown = set(self.ids_opts) - {'C', 'tol', 'max_newton', 'pass_fn'}
            if unknown:
                raise ValueError(f'EvalLoop: unknown pids_uids option(s) {sorted(unknown)}')
        if kid or pids_uids:                # one pair of row buffers serves both
            self.kid_local = tuple(torch.zeros((n_local, fid_dim), dtype=torch.float32, device=shard.device) for _ in range(2))
        self.is_parts = PerStream((lambda: new_accumulator(self.is_opts['num_splits'], self.is_opts['num_classes'], shard.device))
                                  if inception_score else None, shard.device)
        if inception_score:
            if feature_fn is None:
                raise ValueError('EvalLoop: inception_score needs a feature_fn (the detector with its classifier head)')
            self.is_opts = opts = {'num_splits': 10, **(inception_score if isinstance(inception_score, dict) else {})}
            unknown = set(opts) - {'num_splits', 'num_classes', 'no_output_bias', 'accumulate_fn'}
            if unknown:
                raise ValueError(f'EvalLoop: unknown inception_score option(s) {sorted(unknown)}')
            opts['num_classes'] = opts['num_classes'] if opts.get('num_classes') is not None else getattr(feature_fn, 'num_classes', None)
            if opts['num_classes'] is None:
                raise ValueError('EvalLoop: inception_score needs the class count (feature_fn.num_classes or num_classes=...): the detector '
                                 'has no classifier head')
            # item k of this rank sits at dataset position k * world + rank; positions past n_items are padded duplicates (-1: skipped)
            self.is_splits = torch.tensor([split_of(k * shard.world + shard.rank, shard.n_items, opts['num_splits'])
                                           for k in range(n_local)], dtype=torch.int32).to(shard.device)

    def prepare(self, stream_keys):                             # before the first batch: no side stream creates an accumulator
        for parts in (self.fake, self.real, self.is_parts):
            parts.prepare(stream_keys)

    def add(self, out, real, k0):
        if self.is_opts is None:
            feats = self.feature_fn(out)
        else:                               # the same run's probabilities go into this stream's accumulator
            kw = {'no_output_bias': self.is_opts['no_output_bias']} if 'no_output_bias' in self.is_opts else {}
            feats, probs = self.feature_fn(out, with_probs=True, **kw)
            (self.is_opts.get('accumulate_fn') or is_accumulate)(self.is_parts.here(), probs, self.is_splits[k0:k0 + probs.shape[0]])
        self._side(0, self.fake, feats, k0)
        if self.needs_real:
            self._side(1, self.real, self.feature_fn(real, input_range='pm1'), k0)

    def _side(self, side, moments, feats, k0):
        moments.here().add_shard(feats, k0, self.shard.rank, self.shard.world, self.shard.n_items)
        if self.kid_local is not None:
            self.kid_local[side][k0:k0 + feats.shape[0]].copy_(feats)

    def finish(self, collect):
        for moments in (self.fake, self.real):
            if moments.total() is not None:
                collect.sum_(moments.sum.S)

    def finish_kid(self, collect):
        if self.kid_local is not None:
            self.kid_features, self.kid_local = tuple(collect.rows(t) for t in self.kid_local), None

    def finish_is(self, collect):
        if self.is_parts.parts:
            collect.sum_(self.is_parts.total())

    def fid_value(self):
        fake, real = self.fake.sum, self.real.sum            # FidStats: this rank's after total(), all ranks' after finish()
        if self.fid_tail == 'device' and fake is not None and real is not None:
            self.fid_tail_info = frechet_device(*fake.mean_cov_device()[1:], *real.mean_cov_device()[1:], **self.fid_tail_opts)
            return self.fid_tail_info['fid']
        return fid_from_stats(*fake.mean_cov()[1:], *real.mean_cov()[1:]) if fake is not None and real is not None else None

    def kid_value(self):
        on = self.kid_opts is not None and self.kid_features is not None
        return kid_from_features(*(t.contiguous() for t in self.kid_features), **self.kid_opts) if on else None

    def ids_value(self):
        if self.ids_opts is None or self.kid_features is None:
            return None
        fake, real = (t.contiguous() for t in self.kid_features)
        res = ids_from_features(real, fake, **self.ids_opts)
        return res['uids'], res['pids']

    def is_value(self):
        return is_from_accumulator(self.is_parts.sum) if self.is_parts.sum is not None else None


class PerImageColumns:
    """``metrics=('psnr', 'ssim')`` (or a subset) adds the image-quality evaluators of the reference (eva_psnr.py / eva_ssim.py on the evaluator batch
    of shgan_default.py:279-291): per batch one HIP launch pair (image_metrics.py) writes the per-image values of the composite against ``real`` into
    a per-rank float64 buffer at the batch's position; ``metrics_fn(pred, gt, window_size, psnr_out, ssim_out)`` replaces the kernel (CPU tests).
    ``lpips=net`` adds eva_lpips.py: any callable ``lpips(pred_u8, real, out=slice)`` -- ``lpips.Lpips`` on the device, a torch stand-in in the CPU
    tests -- that writes the batch's float64 values into ``out``, this rank's NaN-initialised ``[n_local]`` ``lpips_values`` at the batch's shard
    position.  ``finish`` all-gathers all columns at once and sets ``image_metrics`` (the reference's ``compute()``: {'psnr': mean over exactly
    ``n_items``, 'psnr_per_image': [n_items] in dataset order, ...}), with or without kept images."""
    needs_real = True

    def __init__(self, shard, metrics=None, ssim_window=11, metrics_fn=None, lpips=None):
        if lpips is not None and not callable(lpips):
            raise ValueError('EvalLoop: lpips must be a callable lpips(pred_u8, real, out=slice)')
        self.metrics = MetricsAccumulator(len(shard.ids), shard.device, metrics=tuple(metrics), window_size=ssim_window,
                                          metrics_fn=metrics_fn) if metrics else None           # this rank's PSNR / SSIM columns
        self.lpips_fn, self.image_metrics = lpips, None
        self.lpips_values = torch.full((len(shard.ids),), float('nan'), dtype=torch.float64, device=shard.device) if lpips is not None else None

    def add(self, out, real, k0):
        if self.metrics is not None:
            self.metrics.add(out, real, k0)
        if self.lpips_fn is not None:
            self.lpips_fn(out, real, out=self.lpips_values[k0:k0 + out.shape[0]])

    def finish(self, collect):
        values = dict(self.metrics.values) if self.metrics is not None else {}
        if self.lpips_fn is not None:
            values['lpips'] = self.lpips_values
        full = collect.rows(torch.stack(list(values.values()), dim=1), arrange=False)          # [world, n_local, M] float64
        self.image_metrics = finish_metrics({m: full[:, :, j] for j, m in enumerate(values)}, collect.n_items)


class PrecisionRecall:
    """``pr=dict(detector=vgg, nhood_size=3)``: the improved precision and recall (stylegan_metrics/precision_recall.py, ``pr50k3_full``; independent
    of ``feature_fn``): per batch ``detector(images)`` and ``detector(real, input_range='pm1')`` (``vgg16.Vgg16Features``, or any callable of that
    form) are rounded to float16 into two per-rank buffers ``local`` ``[n_local, dim]`` at the batch's shard position -- one real per fake; ``dim`` is
    ``detector.dim`` or the dict's ``dim``.  ``finish`` gathers them to exactly ``n_items`` rows per side in dataset order (``pr_features``) and
    ``pr_value()`` -> (precision, recall), fakes against reals, runs precision_recall.pr_from_features on them on this device (the manifold sweep is
    not sharded over the ranks; ``kernels_fn`` in the dict replaces the kernels: CPU tests)."""
    needs_real = True

    def __init__(self, shard, pr):
        if not isinstance(pr, dict):
            raise ValueError('EvalLoop: pr must be a dict(detector=..., nhood_size=3)')
        self.pr_opts = {'nhood_size': 3, **pr}
        unknown = set(self.pr_opts) - {'detector', 'nhood_size', 'dim', 'kernels_fn'}
        if unknown:
            raise ValueError(f'EvalLoop: unknown pr option(s) {sorted(unknown)}')
        self.detector = self.pr_opts.pop('detector', None)
        if not callable(self.detector):
            raise ValueError('EvalLoop: pr needs detector=..., a callable detector(images, input_range=None) -> [B, dim]')
        dim = self.pr_opts.pop('dim', None)
        dim = getattr(self.detector, 'dim', None) if dim is None else dim
        if dim is None:
            raise ValueError('EvalLoop: pr needs the feature width (detector.dim or dim=...)')
        if not 1 <= int(self.pr_opts['nhood_size']) <= 15:
            raise ValueError(f"EvalLoop: pr nhood_size must be 1..15 (got {self.pr_opts['nhood_size']})")
        self.pr_features, self.local = None, tuple(torch.zeros((len(shard.ids), int(dim)), dtype=torch.float16, device=shard.device) for _ in range(2))

    def add(self, out, real, k0):
        self.local[0][k0:k0 + out.shape[0]].copy_(self.detector(out))
        self.local[1][k0:k0 + out.shape[0]].copy_(self.detector(real, input_range='pm1'))

    def finish(self, collect):
        if self.local is not None:
            self.pr_features, self.local = tuple(collect.rows(t) for t in self.local), None

    def pr_value(self):
        fake, real = self.pr_features or (None, None)
        return pr_from_features(real.contiguous(), fake.contiguous(), **self.pr_opts) if real is not None else None


class Diversity:
    """``samples_per_input=K, diversity=net`` (``lpips.Lpips``): how different the K completions of one input are -- per input the mean pairwise
    LPIPS among its K samples (diversity.pairwise_lpips: one trunk pass over the batch's B*K composites, the pair head on the K(K-1)/2 pairs).  Not
    one of the per-batch ``add(out, real, k0)`` evaluators: the loop hands it all K samples, ``add_samples(samples_u8 [B,K,3,R,R], k0)``, which
    writes the batch's float64 values into this rank's NaN-initialised ``[n_local]`` ``values`` at the batch's shard position.  ``finish``
    all-gathers them once to ``per_image`` ``[n_items]`` in dataset order; ``diversity_value()`` is their mean."""
    needs_real = False

    def __init__(self, shard, net, samples_per_input):
        if int(samples_per_input) < 2:
            raise ValueError('EvalLoop: diversity needs samples_per_input >= 2 (the pairs among the samples of one input)')
        self.net, self.k, self.per_image = net, int(samples_per_input), None
        self.values = torch.full((len(shard.ids),), float('nan'), dtype=torch.float64, device=shard.device)

    def add(self, out, real, k0):               # (sample 0 alone says nothing about diversity)
        pass

    def add_samples(self, samples, k0):
        from .diversity import pairwise_lpips
        pairwise_lpips(self.net, samples, out=self.values[k0:k0 + samples.shape[0]])

    def finish(self, collect):
        self.per_image = collect.rows(self.values)

    def diversity_value(self):
        return float(self.per_image.mean()) if self.per_image is not None else None
