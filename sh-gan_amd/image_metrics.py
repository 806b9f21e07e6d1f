"""Per-image PSNR and SSIM of the evaluation loop (reference lib/evaluator/eva_psnr.py with ``for_dataset=None, rgb_range=1`` and
lib/evaluator/eva_ssim.py, ``compute_ssim(..., size_average=False)``), computed on the device by csrc/image_metrics.hip.

The reference's evaluator batch (shgan_default.py:279-291) holds ``pred = fake_u8 / 255`` and ``gt = (real + 1) / 2`` on the host; here
both forms are made inside the kernel's load from what the loop already has on the device: the uint8 composite and the feeder's
``real`` (float32 in [-1, 1], or the decoded uint8 pixels mapped through ``kernels.u8_value_table``).

    psnr, ssim = image_metrics(pred_u8, real)                         # float64 [B] each, on the device
    acc = MetricsAccumulator(n_local, device); acc.add(pred, real, k0)  # a rank's per-image values at its shard positions
    finish_metrics(per_rank_values, n_items)                          # dataset order (zipzap), [0:sample_n], mean"""
import numpy as np
import torch

from . import _lib, kernels
from ._lib import ShgError, check

METRICS = ('psnr', 'ssim')
_PRED_LUT = {}


def pred_value_table(device, dtype=torch.float32):
    """Value of every uint8 code of the composite as the reference's evaluators see it: ``numpy u8 / 255`` -- float64 for PSNR, rounded
    to float32 for SSIM (``torch.FloatTensor``).  The kernel takes the float64 table and rounds it itself."""
    key = (str(device), dtype)
    if key not in _PRED_LUT:
        _PRED_LUT[key] = torch.from_numpy(np.arange(256, dtype=np.float64) / 255).to(dtype).to(device)
    return _PRED_LUT[key]


def _operand(L, t, name, lut):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ShgError(f'image_metrics: {name} must reside on a HIP (cuda) device: there is no CPU path')
    if t.dtype == torch.uint8:
        return L.req(t, name, dtype=torch.uint8), L.req(lut, name + '_lut', dtype=lut.dtype)
    if t.dtype != torch.float32:
        raise ShgError(f'image_metrics: {name} must be uint8 or float32 (got {t.dtype})')
    return L.req(t, name), None


def scratch_bytes(b, h, w, window_size=11):
    return int(_lib.get_lib().shg_image_metrics_scratch_bytes(int(b), int(h), int(w), int(window_size)))


def image_metrics(pred, gt, window_size=11, gt_range='pm1', psnr_only=False, psnr_out=None, ssim_out=None):
    """pred [B,C,H,W]: uint8 composite (value u8/255) or float32 in [0, 1]; gt [B,C,H,W]: ``gt_range='pm1'`` float32 in [-1, 1] or uint8
    decoded pixels (value ``u8_value_table``), mapped to (v + 1) / 2; ``gt_range='unit'``: float32 in [0, 1] or uint8 (value u8/255 in
    float32) taken as they are.  PSNR takes pred in float64 and gt in float32, as the reference's evaluator batch holds them.  -> (psnr [B] float64, ssim [B] float64 | None when ``psnr_only``), on the device, enqueued on the current stream.
    ``psnr_out`` / ``ssim_out``: float64 [B] views to write into (e.g. a slice of a per-rank buffer)."""
    if gt_range not in ('pm1', 'unit'):
        raise ShgError(f"image_metrics: gt_range must be 'pm1' or 'unit' (got {gt_range!r})")
    if not (isinstance(pred, torch.Tensor) and isinstance(gt, torch.Tensor)) or pred.ndim != 4 or tuple(pred.shape) != tuple(gt.shape):
        raise ShgError('image_metrics: pred and gt must be [B,C,H,W] tensors of one shape')
    ws = int(window_size)
    if ws < 1 or ws > 31 or ws % 2 == 0:
        raise ShgError(f'image_metrics: window_size must be odd and in [1, 31] (got {ws}): an even window changes the output size')
    L = kernels._Launch()
    dev = pred.device if pred.is_cuda else None
    p, plut = _operand(L, pred, 'pred', pred_value_table(dev, torch.float64) if dev is not None else None)
    if gt_range == 'pm1':
        gt_lut = kernels.u8_value_table(L.dev) if gt.is_cuda and gt.dtype == torch.uint8 else None
        gs, gb = 0.5, 0.5
    else:
        gt_lut = pred_value_table(L.dev) if gt.is_cuda and gt.dtype == torch.uint8 else None
        gs, gb = 1.0, 0.0
    g, glut = _operand(L, gt, 'gt', gt_lut)
    b, c, h, w = p.shape
    psnr = psnr_out if psnr_out is not None else torch.empty(b, dtype=torch.float64, device=L.dev)
    ssim = None if psnr_only else (ssim_out if ssim_out is not None else torch.empty(b, dtype=torch.float64, device=L.dev))
    for name, o in (('psnr_out', psnr), ('ssim_out', ssim)):
        if o is not None:
            L.req(o, name, dtype=torch.float64)
            if o.numel() != b or not o.is_contiguous():
                raise ShgError(f'image_metrics: {name} must be a contiguous float64 [{b}] tensor')
    nbytes = scratch_bytes(b, h, w, ws)
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=L.dev)
    with L:
        check(_lib.get_lib().shg_image_metrics(kernels._ptr(p), kernels._ptr(plut), 1.0, 0.0, kernels._ptr(g), kernels._ptr(glut), gs, gb,
                                               b, c, h, w, ws, int(bool(psnr_only)), kernels._ptr(scratch), nbytes, kernels._ptr(psnr),
                                               kernels._ptr(ssim), L.stream()), 'image_metrics')
    return psnr, ssim


class MetricsAccumulator:
    """This rank's per-image values at their shard positions: ``values[name]`` float64 [n_local] (position k = the k-th item of the rank's
    ``DistributedSampler(extend=True)`` list).  Every batch writes its own slice, so batches on different streams share no accumulator.
    ``metrics_fn(pred, gt, window_size, psnr_out, ssim_out)`` replaces the HIP kernel (the CPU tests inject a torch stand-in)."""

    def __init__(self, n_local, device, metrics=METRICS, window_size=11, metrics_fn=None):
        bad = [m for m in metrics if m not in METRICS]
        if bad or not metrics:
            raise ShgError(f'MetricsAccumulator: metrics must be a non-empty subset of {METRICS} (got {tuple(metrics)})')
        ws = int(window_size)
        if ws < 1 or ws > 31 or ws % 2 == 0:
            raise ShgError(f'MetricsAccumulator: window_size must be odd and in [1, 31] (got {ws})')
        self.metrics, self.window_size, self.fn = tuple(metrics), ws, metrics_fn
        dev = torch.device(device)
        self.values = {m: torch.full((int(n_local),), float('nan'), dtype=torch.float64, device=dev) for m in METRICS if m in self.metrics}

    def add(self, pred, gt, k0):
        b = pred.shape[0]
        p_out = self.values['psnr'][k0:k0 + b] if 'psnr' in self.values else None
        s_out = self.values['ssim'][k0:k0 + b] if 'ssim' in self.values else None
        if self.fn is not None:
            self.fn(pred, gt, self.window_size, p_out, s_out)
            return
        if p_out is None:           # SSIM only: PSNR costs nothing extra in the same pass; it goes to a throw-away buffer
            p_out = torch.empty(b, dtype=torch.float64, device=pred.device)
        image_metrics(pred, gt, window_size=self.window_size, psnr_only=s_out is None, psnr_out=p_out, ssim_out=s_out)


def finish_metrics(per_rank, n_items):
    """The reference's ``compute()`` (eva_psnr.py / eva_ssim.py): per_rank {name: [world, n_local]} float64 (rank r's k-th value at
    [r, k]) -> {name: mean over the first ``n_items`` in dataset order, name + '_per_image': [n_items]}.  Dataset order is the zipzap
    re-interleave (item k*world + r); the padded duplicates of ``DistributedSampler(extend=True)`` fall beyond ``n_items``."""
    from .eval_harness import zipzap_device
    out = {}
    for name, full in per_rank.items():
        vals = zipzap_device(full, int(n_items))
        out[name + '_per_image'] = vals
        out[name] = float(vals.double().mean().item())
    return out

