"""The ADA augmentation pipe on the device (StyleGAN2-ADA's ``AugmentPipe``; the hook of ``stylegan_default_loss.py:47-48`` and the
controller of ``stylegan_default.py:397-400``, which the reference keeps but ships no pipe for).

``AugmentPipe`` has ADA's constructor keywords and defaults for the blit, geometry and colour categories.  One call is two launches
(``csrc/ada.hip``): ``shg_ada_params_f32`` turns the draws and the probability ``p`` -- both on the device -- into a geometry matrix, a
colour matrix per sample and the batch-wide reflect-pad margins, and ``shg_ada_apply_f32`` runs ADA's chain reflect-pad -> x2 wavelet
upsampling -> bilinear affine resampling -> x2 decimation -> colour matrix over the images in one pass.  No shape depends on a draw and
nothing is read back, so the pipe can be captured into a HIP graph (``train_stage.PhaseGraphs``): a replay draws again and reads the
current ``p``.

Draw layout.  ``draws = (u, g)``, ``u`` [N, 24] uniform in [0, 1), ``g`` [N, 8] standard normal, one row per image; value column(s),
then gate column, in ADA's order:

    xflip u0 | u1        rotate90 u2 | u3      xint u4 u5 | u6       scale g0 | u7      pre-rotation u8 | u9     aniso g1 | u10
    post-rotation u11 | u12      xfrac g2 g3 | u13      brightness g4 | u14      contrast g5 | u15      lumaflip u16 | u17
    hue u18 | u19        saturation g6 | u20           (u21..u23 and g7 are not read)

A transform fires for an image when its gate column is below ``multiplier * p`` (rotations: ``1 - sqrt(1 - rotate * p)`` each).  The
draws are not those of ADA's many small ``torch.rand`` calls: the distribution is the same, the random stream is not.

Channels.  Geometry moves every channel.  Colour acts on ``color_channels = (first, count)``, count 1 or 3; the default is all channels
for C = 1 or 3 and channels 1..3 for C = 4 -- the critic input ``cat([mask - 0.5, img])`` of ``losses.InpaintingLoss``, whose mask channel
keeps its values.  ``imgfilter``, ``noise`` and ``cutout`` are accepted as 0 only by ``AugmentPipe``; ``FullAugmentPipe`` (at the end of this
file, ``csrc/ada_tail.hip``) runs them after the colour stage.

The operator is linear in the image (plus the colour offset); its backward is ``shg_ada_apply_adjoint_f32``, whose backward is the forward
kernel again, so R1 (``create_graph=True``) differentiates through it.  The adjoint accumulates with float atomics whose order is not fixed:
gradients through the pipe are not bit-reproducible from run to run.

``deterministic=True`` (``ada_apply``, ``ada_apply_adjoint``, ``AugmentPipe``, ``FullAugmentPipe``; off by default) takes the gather form of
the adjoint instead, ``shg_ada_apply_adjoint_gather_f32``: two launches without atomics and a workspace of the sample grid's size; the
gradient is the same bits on every run and for every batch a sample is part of (given the margins).  The forward is the same launch either
way.  The one exception is decided per sample on the device: a singular matrix, one that magnifies more than about 16-fold or one with a
non-finite or huge (2^24) entry is left to the scatter kernel -- that sample's gradient is correct but not bit-reproducible (the parameter kernel
cannot produce such a matrix from finite draws)."""
import ctypes

import numpy as np
import torch

from . import _lib

N_UNIFORM, N_NORMAL = 24, 8

# sym6 low-pass (ADA's wavelets['sym6']), normalised to sum 1 below
_SYM6 = (0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633, 0.4910559419267466, 0.787641141030194,
         0.3379294217276218, -0.07263752278646252, -0.021060292512300564, 0.04472490177066578, 0.0017677118642428036, -0.007800708325034148)

_GEOM = ('xflip', 'rotate90', 'xint', 'scale', 'rotate', 'aniso', 'xfrac')
_COLOR = ('brightness', 'contrast', 'lumaflip', 'hue', 'saturation')
_STDS = ('xint_max', 'scale_std', 'rotate_max', 'aniso_std', 'xfrac_std', 'brightness_std', 'contrast_std', 'hue_max', 'saturation_std')

# ADA's named sets (train.py: augpipe_specs) restricted to the categories built here
AUGPIPE_SPECS = {
    'blit': dict(xflip=1, rotate90=1, xint=1),
    'geom': dict(scale=1, rotate=1, aniso=1, xfrac=1),
    'color': dict(brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1),
    'bg': dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1),
    'bgc': dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1),
}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check_image(x, what):
    if not (isinstance(x, torch.Tensor) and x.ndim == 4 and x.dtype == torch.float32 and x.is_cuda):
        raise _lib.ShgError(f'{what}: a float32 [N, C, H, W] tensor on the device is required (got '
                            f'{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}, {getattr(x, "dtype", None)}, '
                            f'{getattr(x, "device", None)})')


def ada_params(u, g, p, cfg, H, W):
    """-> (G_inv [N,3,3], Cm [N,3,4], margins int32 [4] = mx0, my0, mx1, my1) on the device, from draws u [N,24], g [N,8] and the
    one-element tensor p; ``cfg`` an ``_lib.AdaConfig``.  One launch, nothing read back."""
    n = u.shape[0]
    if tuple(u.shape) != (n, N_UNIFORM) or tuple(g.shape) != (n, N_NORMAL) or u.dtype != torch.float32 or g.dtype != torch.float32:
        raise _lib.ShgError(f'ada_params: draws must be float32 u [N, {N_UNIFORM}] and g [N, {N_NORMAL}] (got {tuple(u.shape)}, {tuple(g.shape)})')
    if not (u.is_cuda and g.is_cuda and p.is_cuda and p.dtype == torch.float32 and p.numel() == 1):
        raise _lib.ShgError('ada_params: u, g and the float32 scalar p must live on the device')
    u, g = u.contiguous(), g.contiguous()
    with torch.cuda.device(u.device):
        G = torch.empty([n, 3, 3], dtype=torch.float32, device=u.device)
        Cm = torch.empty([n, 3, 4], dtype=torch.float32, device=u.device)
        margins = torch.empty([4], dtype=torch.int32, device=u.device)
        _lib.check(_lib.get_lib().shg_ada_params_f32(_ptr(u), _ptr(g), _ptr(p), ctypes.byref(cfg), _ptr(G), _ptr(Cm), _ptr(margins), n, int(H),
                                                     int(W), _stream(u)), 'ada_params')
    return G, Cm, margins


def _launch(adjoint, x, G, Cm, margins, geom, color, bias, deterministic=False):
    _check_image(x, 'ada_apply')
    n, c, h, w = x.shape
    first, count = color if color is not None else (0, 0)
    if geom and (G is None or margins is None or tuple(G.shape) != (n, 3, 3) or G.dtype != torch.float32 or margins.dtype != torch.int32
                 or margins.numel() != 4 or G.device != x.device or margins.device != x.device):
        raise _lib.ShgError('ada_apply: geometry needs G_inv float32 [N,3,3] and margins int32 [4] on the image device')
    if count and (Cm is None or tuple(Cm.shape) != (n, 3, 4) or Cm.dtype != torch.float32 or Cm.device != x.device):
        raise _lib.ShgError('ada_apply: colour needs the colour matrix float32 [N,3,4] on the image device')
    x = x.contiguous()
    G = G.contiguous() if geom else None
    Cm = Cm.contiguous() if count else None
    margins = margins.contiguous() if geom else None
    with torch.cuda.device(x.device):
        lib = _lib.get_lib()
        gather = bool(adjoint and deterministic)
        # the scatter adjoint accumulates into its output with atomics; the gather form writes every element
        y = torch.zeros_like(x) if adjoint and geom and not gather else torch.empty_like(x)
        if gather:
            nbytes = int(lib.shg_ada_adjoint_gather_workspace_bytes(n, c, h, w)) if geom else 0
            ws = torch.empty([nbytes // 4], dtype=torch.float32, device=x.device) if nbytes else None
            rc = lib.shg_ada_apply_adjoint_gather_f32(_ptr(x), _ptr(G), _ptr(Cm), _ptr(margins), _ptr(y), _ptr(ws), nbytes, n, c, h, w, int(geom),
                                                      first, count, _stream(x))
        elif adjoint:
            rc = lib.shg_ada_apply_adjoint_f32(_ptr(x), _ptr(G), _ptr(Cm), _ptr(margins), _ptr(y), n, c, h, w, int(geom), first, count, _stream(x))
        else:
            rc = lib.shg_ada_apply_f32(_ptr(x), _ptr(G), _ptr(Cm), _ptr(margins), _ptr(y), n, c, h, w, int(geom), first, count, int(bias),
                                       _stream(x))
        _lib.check(rc, 'ada_apply_adjoint' if adjoint else 'ada_apply')
    return y


class _AdaApplyFn(torch.autograd.Function):
    """y = A x (+ the colour offset when ``bias``); backward: the adjoint kernel."""

    @staticmethod
    def forward(ctx, x, G, Cm, margins, geom, color, bias, deterministic=False):
        ctx.save_for_backward(G, Cm, margins)
        ctx.cfg = (geom, color, bool(deterministic))
        return _launch(False, x.detach(), G, Cm, margins, geom, color, bias)

    @staticmethod
    def backward(ctx, gy):
        G, Cm, margins = ctx.saved_tensors
        geom, color, deterministic = ctx.cfg
        return _AdaAdjointFn.apply(gy, G, Cm, margins, geom, color, deterministic), None, None, None, None, None, None, None


class _AdaAdjointFn(torch.autograd.Function):
    """gx = A^T gy; backward: the forward kernel without the offset (the operator is linear)."""

    @staticmethod
    def forward(ctx, gy, G, Cm, margins, geom, color, deterministic=False):
        ctx.save_for_backward(G, Cm, margins)
        ctx.cfg = (geom, color, bool(deterministic))
        return _launch(True, gy.detach(), G, Cm, margins, geom, color, False, deterministic)

    @staticmethod
    def backward(ctx, ggx):
        G, Cm, margins = ctx.saved_tensors
        geom, color, deterministic = ctx.cfg
        return _AdaApplyFn.apply(ggx, G, Cm, margins, geom, color, False, deterministic), None, None, None, None, None, None


def ada_apply(x, G_inv=None, Cm=None, margins=None, color_channels=None, deterministic=False):
    """The pipe's image operator on given parameters (differentiable in ``x``, twice): geometry when ``G_inv`` [N,3,3] and ``margins``
    int32 [4] are given, colour on ``color_channels = (first, count)`` when ``Cm`` [N,3,4] is.  Neither: ``x`` itself.
    ``deterministic``: the gradient takes the gather form of the adjoint (same bits on every run); the forward is the same launch."""
    geom, color = G_inv is not None, (tuple(int(v) for v in color_channels) if Cm is not None else None)
    if not geom and color is None:
        return x
    if color is not None:
        _check_color(color, x.shape[1])
    return _AdaApplyFn.apply(x, G_inv, Cm, margins, geom, color, True, bool(deterministic))


def ada_apply_adjoint(gy, G_inv=None, Cm=None, margins=None, color_channels=None, deterministic=False):
    """The transpose of ``ada_apply``'s linear part; ``deterministic``: in gather form, without atomics."""
    geom, color = G_inv is not None, (tuple(int(v) for v in color_channels) if Cm is not None else None)
    if not geom and color is None:
        return gy
    if color is not None:
        _check_color(color, gy.shape[1])
    return _AdaAdjointFn.apply(gy, G_inv, Cm, margins, geom, color, bool(deterministic))


def _check_color(color, c):
    if len(color) != 2 or color[1] not in (1, 3) or color[0] < 0 or color[0] + color[1] > c:
        raise ValueError(f'color_channels must be (first, count) with count 1 or 3 inside the {c} channels (got {color})')


def default_color_channels(c):
    """(first, count) for C channels: all of 1 or 3, channels 1..3 of 4 (mask + RGB); any other C needs an explicit pair."""
    if c in (1, 3):
        return (0, c)
    if c == 4:
        return (1, 3)
    raise ValueError(f'AugmentPipe: {c} channels need an explicit color_channels=(first, count)')


class AugmentPipe(torch.nn.Module):
    def __init__(self, xflip=0, rotate90=0, xint=0, xint_max=0.125,
                 scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2, xfrac_std=0.125,
                 brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1, saturation_std=1,
                 imgfilter=0, imgfilter_bands=(1, 1, 1, 1), imgfilter_std=1, noise=0, cutout=0, noise_std=0.1, cutout_size=0.5,
                 color_channels=None, deterministic=False):
        super().__init__()
        self.deterministic = bool(deterministic)     # gradients through the geometry in gather form (a plain attribute, not a buffer)
        for name, value in (('imgfilter', imgfilter), ('noise', noise), ('cutout', cutout)):
            if float(value) != 0:
                raise NotImplementedError(f'AugmentPipe: {name} is not part of the HIP path (only {name}=0 is accepted)')
        loc = locals()
        for name in _GEOM + _COLOR + _STDS:
            setattr(self, name, float(loc[name]))
        if color_channels is not None:
            color_channels = tuple(int(v) for v in color_channels)
            if len(color_channels) != 2 or color_channels[1] not in (1, 3) or color_channels[0] < 0:
                raise ValueError(f'AugmentPipe: color_channels must be (first, count) with count 1 or 3 (got {color_channels})')
        self.color_channels = color_channels
        self.register_buffer('p', torch.ones([]))           # overall multiplier of the probabilities (AdaController adjusts it)
        f = np.asarray(_SYM6, dtype=np.float64)
        self.register_buffer('Hz_geom', torch.as_tensor(f / f.sum(), dtype=torch.float32))     # ADA's state_dict key; the kernel holds the taps

    @property
    def geometry_on(self):
        return any(getattr(self, n) > 0 for n in _GEOM)

    @property
    def color_on(self):
        return any(getattr(self, n) > 0 for n in _COLOR)

    def _color_for(self, c):
        color = self.color_channels if self.color_channels is not None else default_color_channels(c)
        _check_color(color, c)
        return color

    def _config(self, count):
        cfg = _lib.AdaConfig()
        for name in _GEOM + _COLOR + _STDS:
            setattr(cfg, name, getattr(self, name))
        if count == 1:
            cfg.hue = cfg.saturation = 0.0
        cfg.color_count = count
        return cfg

    def draw(self, n, device=None):
        """Fresh draws for n images: (u [n,24] uniform, g [n,8] normal) on the device; one generator call each (graph-safe)."""
        device = self.p.device if device is None else device
        return torch.rand([n, N_UNIFORM], device=device), torch.randn([n, N_NORMAL], device=device)

    def params(self, draws, c, h, w):
        """-> (G_inv, Cm, margins, color) for a batch of [len(u), c, h, w] images on the given draws."""
        color = self._color_for(c)
        u, g = draws
        G, Cm, margins = ada_params(u, g, self.p.reshape(1), self._config(color[1]), h, w)
        return G, Cm, margins, color

    def forward(self, images, draws=None):
        _check_image(images, 'AugmentPipe')
        n, c, h, w = images.shape
        color = self._color_for(c)
        geom, col = self.geometry_on, self.color_on
        if not geom and not col:
            return images
        if draws is None:
            draws = self.draw(n, images.device)
        G, Cm, margins, _ = self.params(draws, c, h, w)
        return ada_apply(images, G if geom else None, Cm if col else None, margins if geom else None, color, deterministic=self.deterministic)


class AdaController:
    """The ADA heuristic of stylegan_default.py:397-400: ``update`` once per iteration with the signs of the real logits
    (``loss.stats['Loss/signs/real']``); sums and counts stay on the tensor's device, and every ``ada_interval`` iterations one small
    read-back (after an all-reduce when ``torch.distributed`` is initialised) moves ``pipe.p`` by
    ``sign(mean - ada_target) * batch_size * ada_interval / (ada_kimg * 1000)``, floored at 0."""

    def __init__(self, pipe, ada_target=0.6, ada_interval=4, ada_kimg=500):
        self.pipe, self.ada_target, self.ada_interval, self.ada_kimg = pipe, float(ada_target), int(ada_interval), float(ada_kimg)
        if self.ada_interval < 1:
            raise ValueError('AdaController: ada_interval >= 1')
        self.acc = None
        self.iters = 0
        self.last_mean = None

    def state_dict(self):
        """What a resumed run needs to continue the heuristic where it stood (``pipe.p`` is a buffer of the pipe and travels with it)."""
        return {'acc': None if self.acc is None else self.acc.detach().clone(), 'iters': int(self.iters), 'last_mean': self.last_mean}

    def load_state_dict(self, state):
        acc = state['acc']
        self.acc = None if acc is None else acc.detach().clone().to(self.pipe.p.device)
        self.iters = int(state['iters'])
        self.last_mean = state['last_mean']

    @torch.no_grad()
    def update(self, signs, batch_size):
        """-> the adjustment applied to p at this call (0.0 between intervals)."""
        signs = signs.detach().to(torch.float32).reshape(-1)
        part = torch.stack([signs.sum(), torch.full([], float(signs.numel()), device=signs.device)])
        self.acc = part if self.acc is None else self.acc.to(part.device) + part
        self.iters += 1
        if self.iters % self.ada_interval != 0:
            return 0.0
        acc = self.acc
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(acc)
        total, count = (float(v) for v in acc.cpu())
        self.acc = None
        self.last_mean = total / max(count, 1.0)
        adjust = float(np.sign(self.last_mean - self.ada_target)) * (batch_size * self.ada_interval) / (self.ada_kimg * 1000)
        p = self.pipe.p
        p.copy_((p + adjust).clamp_(min=0))
        return adjust


# ---- the tail of ADA's pipe: image-space filter, noise, cutout (csrc/ada_tail.hip) ---------------------------------------------------------
# ``FullAugmentPipe`` is ``AugmentPipe`` followed by ADA's remaining three categories, in ADA's order.  One more parameter launch
# (``shg_ada_tail_params_f32``: per-sample taps g @ Hz_fbank [N,43], sigma [N], the cutout box [N,4]) and one more fused launch
# (``shg_ada_tail_apply_f32``).  Draw layout of the tail, ``ut`` [N, 8] uniform and ``gt`` [N, 5] normal, value | gate:
#
#     imgfilter band i (0..3) gt_i | ut_i        noise gt4 | ut4        cutout centre ut6 (x), ut7 (y) | ut5
#
# and the noise field ``z`` [N, count, H, W], standard normal.  The filter and the noise act on ``color_channels`` (the colour stage's rule
# and default: the mask channel of the C = 4 critic input is neither filtered nor given noise); the cutout multiplies every channel.  The
# transpose (``shg_ada_tail_adjoint_f32``) is a gather without atomics: gradients through the tail are the same bits on every run.
N_UNIFORM_TAIL, N_NORMAL_TAIL, TAIL_TAPS = 8, 5, 43

_SYM2 = (-0.12940952255092145, 0.22414386804185735, 0.836516303737469, 0.48296291314469025)       # ADA's wavelets['sym2']
_TAIL = ('imgfilter', 'noise', 'cutout')

_BGCF = dict(AUGPIPE_SPECS['bgc'], imgfilter=1)
# ADA's named sets (train.py: augpipe_specs), all of them
AUGPIPE_SPECS_FULL = dict(
    AUGPIPE_SPECS,
    filter=dict(imgfilter=1),
    noise=dict(noise=1),
    cutout=dict(cutout=1),
    bgcf=_BGCF,
    bgcfn=dict(_BGCF, noise=1),
    bgcfnc=dict(_BGCF, noise=1, cutout=1),
)


def hz_fbank():
    """ADA's ``Hz_fbank``, float64 [4, 43]: the sym2 low-pass and its mirror, three rounds of zero-stuffing and convolution."""
    lo = np.asarray(_SYM2, dtype=np.float64)
    hi = lo * ((-1.0) ** np.arange(lo.size))
    lo2 = np.convolve(lo, lo[::-1]) / 2
    hi2 = np.convolve(hi, hi[::-1]) / 2
    fb = np.eye(4, 1)
    for i in range(1, 4):
        fb = np.dstack([fb, np.zeros_like(fb)]).reshape(4, -1)[:, :-1]
        fb = np.stack([np.convolve(row, lo2) for row in fb])
        fb[i, (fb.shape[1] - hi2.size) // 2:(fb.shape[1] + hi2.size) // 2] += hi2
    return fb


def ada_tail_params(ut, gt, p, cfg):
    """-> (Hz [N,43], sigma [N], cut [N,4] = cx, cy, half_w, half_h) on the device, from draws ut [N,8], gt [N,5] and the one-element tensor
    p; ``cfg`` an ``_lib.AdaTailConfig``.  One launch, nothing read back."""
    n = ut.shape[0]
    if (tuple(ut.shape) != (n, N_UNIFORM_TAIL) or tuple(gt.shape) != (n, N_NORMAL_TAIL) or ut.dtype != torch.float32
            or gt.dtype != torch.float32):
        raise _lib.ShgError(f'ada_tail_params: draws must be float32 ut [N, {N_UNIFORM_TAIL}] and gt [N, {N_NORMAL_TAIL}] (got '
                            f'{tuple(ut.shape)}, {tuple(gt.shape)})')
    if not (ut.is_cuda and gt.is_cuda and p.is_cuda and p.dtype == torch.float32 and p.numel() == 1):
        raise _lib.ShgError('ada_tail_params: ut, gt and the float32 scalar p must live on the device')
    ut, gt = ut.contiguous(), gt.contiguous()
    with torch.cuda.device(ut.device):
        Hz = torch.zeros([n, TAIL_TAPS], dtype=torch.float32, device=ut.device)
        sigma = torch.zeros([n], dtype=torch.float32, device=ut.device)
        cut = torch.zeros([n, 4], dtype=torch.float32, device=ut.device)
        _lib.check(_lib.get_lib().shg_ada_tail_params_f32(_ptr(ut), _ptr(gt), _ptr(p), ctypes.byref(cfg), _ptr(Hz), _ptr(sigma), _ptr(cut), n,
                                                          _stream(ut)), 'ada_tail_params')
    return Hz, sigma, cut


def _tail_launch(adjoint, x, Hz, sigma, z, cut, color, bias):
    _check_image(x, 'ada_tail_apply')
    n, c, h, w = x.shape
    first, count = color if color is not None else (0, 0)

    def ok(t, shape):
        return t is None or (tuple(t.shape) == shape and t.dtype == torch.float32 and t.device == x.device)
    if not (ok(Hz, (n, TAIL_TAPS)) and ok(sigma, (n,)) and ok(z, (n, count, h, w)) and ok(cut, (n, 4))):
        raise _lib.ShgError(f'ada_tail_apply: Hz [N,{TAIL_TAPS}], sigma [N], z [N,{count},H,W] and cut [N,4] must be float32 on the image device')
    x = x.contiguous()
    Hz, sigma, z, cut = (t.contiguous() if t is not None else None for t in (Hz, sigma, z, cut))
    with torch.cuda.device(x.device):
        # zero-filled although the kernels write every element (tests/test_gpu_ada_tail.py runs them into poisoned buffers): an
        # uninitialised allocation of the package needs a poison-fill case in tests/test_gpu_alloc_fill.py, and the tail has none
        y = torch.zeros_like(x)
        lib = _lib.get_lib()
        if adjoint:
            rc = lib.shg_ada_tail_adjoint_f32(_ptr(x), _ptr(Hz), _ptr(cut), _ptr(y), n, c, h, w, first, count, _stream(x))
        else:
            rc = lib.shg_ada_tail_apply_f32(_ptr(x), _ptr(Hz), _ptr(sigma), _ptr(z), _ptr(cut), _ptr(y), n, c, h, w, first, count, int(bias),
                                            _stream(x))
        _lib.check(rc, 'ada_tail_adjoint' if adjoint else 'ada_tail_apply')
    return y


class _AdaTailApplyFn(torch.autograd.Function):
    """y = A x (+ sigma z when ``bias``); backward: the adjoint kernel."""

    @staticmethod
    def forward(ctx, x, Hz, sigma, z, cut, color, bias):
        ctx.save_for_backward(Hz, cut)
        ctx.color = color
        return _tail_launch(False, x.detach(), Hz, sigma, z, cut, color, bias)

    @staticmethod
    def backward(ctx, gy):
        Hz, cut = ctx.saved_tensors
        if Hz is None and cut is None:               # noise alone: the linear part is the identity
            return gy, None, None, None, None, None, None
        return _AdaTailAdjointFn.apply(gy, Hz, cut, ctx.color), None, None, None, None, None, None


class _AdaTailAdjointFn(torch.autograd.Function):
    """gx = A^T gy; backward: the forward kernel without the noise term (the operator is linear)."""

    @staticmethod
    def forward(ctx, gy, Hz, cut, color):
        ctx.save_for_backward(Hz, cut)
        ctx.color = color
        return _tail_launch(True, gy.detach(), Hz, None, None, cut, color, False)

    @staticmethod
    def backward(ctx, ggx):
        Hz, cut = ctx.saved_tensors
        if Hz is None and cut is None:
            return ggx, None, None, None
        return _AdaTailApplyFn.apply(ggx, Hz, None, None, cut, ctx.color, False), None, None, None


def _tail_color(Hz, z, color_channels, c):
    if Hz is None and z is None:
        return None
    color = tuple(int(v) for v in color_channels) if color_channels is not None else default_color_channels(c)
    _check_color(color, c)
    return color


def ada_tail_apply(x, Hz=None, sigma=None, z=None, cut=None, color_channels=None):
    """The tail's image operator on given parameters (differentiable in ``x``, twice): ``mask * (fir(x) + sigma z)`` on ``color_channels =
    (first, count)``, ``mask * x`` on the others.  The filter runs when ``Hz`` [N,43] is given, the noise when ``sigma`` [N] and ``z``
    [N,count,H,W] are, the cutout when ``cut`` [N,4] is.  None of them: ``x`` itself."""
    if (sigma is None) != (z is None):
        raise ValueError('ada_tail_apply: the noise needs both sigma and z')
    if Hz is None and z is None and cut is None:
        return x
    return _AdaTailApplyFn.apply(x, Hz, sigma, z, cut, _tail_color(Hz, z, color_channels, x.shape[1]), True)


def ada_tail_apply_adjoint(gy, Hz=None, cut=None, color_channels=None):
    """The transpose of ``ada_tail_apply``'s linear part ``mask * fir``."""
    if Hz is None and cut is None:
        return gy
    return _AdaTailAdjointFn.apply(gy, Hz, cut, _tail_color(Hz, None, color_channels, gy.shape[1]))


class FullAugmentPipe(AugmentPipe):
    """ADA's whole pipe: ``AugmentPipe`` (blit, geometry, colour), then imgfilter, noise and cutout.  ``draws`` is ``(u, g, ut, gt)`` or
    ``(u, g, ut, gt, z)``; without ``z`` a noise field is drawn with one ``torch.randn``.  ``(u, g)`` alone serves while the tail is off."""

    def __init__(self, xflip=0, rotate90=0, xint=0, xint_max=0.125,
                 scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2, xfrac_std=0.125,
                 brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1, saturation_std=1,
                 imgfilter=0, imgfilter_bands=(1, 1, 1, 1), imgfilter_std=1, noise=0, cutout=0, noise_std=0.1, cutout_size=0.5,
                 color_channels=None, deterministic=False):
        super().__init__(xflip=xflip, rotate90=rotate90, xint=xint, xint_max=xint_max, scale=scale, rotate=rotate, aniso=aniso, xfrac=xfrac,
                         scale_std=scale_std, rotate_max=rotate_max, aniso_std=aniso_std, xfrac_std=xfrac_std, brightness=brightness,
                         contrast=contrast, lumaflip=lumaflip, hue=hue, saturation=saturation, brightness_std=brightness_std,
                         contrast_std=contrast_std, hue_max=hue_max, saturation_std=saturation_std, imgfilter=0, noise=0, cutout=0,
                         color_channels=color_channels, deterministic=deterministic)
        self.imgfilter, self.noise, self.cutout = float(imgfilter), float(noise), float(cutout)
        self.imgfilter_bands = tuple(float(v) for v in imgfilter_bands)
        if len(self.imgfilter_bands) != 4:
            raise ValueError(f'FullAugmentPipe: imgfilter_bands must have 4 entries, one per band of Hz_fbank (got {len(self.imgfilter_bands)})')
        self.imgfilter_std, self.noise_std, self.cutout_size = float(imgfilter_std), float(noise_std), float(cutout_size)
        self.register_buffer('Hz_fbank', torch.as_tensor(hz_fbank(), dtype=torch.float32))     # ADA's state_dict key; the kernel holds the taps

    @property
    def tail_on(self):
        return any(getattr(self, n) > 0 for n in _TAIL)

    def _tail_config(self):
        cfg = _lib.AdaTailConfig()
        for name in ('imgfilter', 'imgfilter_std', 'noise', 'noise_std', 'cutout', 'cutout_size'):
            setattr(cfg, name, getattr(self, name))
        cfg.bands[:] = self.imgfilter_bands
        return cfg

    def draw(self, n, device=None):
        """Fresh draws for n images: (u [n,24], g [n,8], ut [n,8], gt [n,5]) on the device; one generator call each (graph-safe)."""
        device = self.p.device if device is None else device
        return super().draw(n, device) + (torch.rand([n, N_UNIFORM_TAIL], device=device), torch.randn([n, N_NORMAL_TAIL], device=device))

    def params(self, draws, c, h, w):
        return super().params(tuple(draws)[:2], c, h, w)

    def tail_params(self, draws):
        """-> (Hz, sigma, cut) of the tail on the draws (u, g, ut, gt[, z])."""
        return ada_tail_params(draws[2], draws[3], self.p.reshape(1), self._tail_config())

    def forward(self, images, draws=None):
        _check_image(images, 'FullAugmentPipe')
        n, c, h, w = images.shape
        color = self._color_for(c)
        tail = self.tail_on
        if not tail and not self.geometry_on and not self.color_on:
            return images
        if draws is None and (self.geometry_on or self.color_on):
            draws = self.draw(n, images.device)
        elif draws is None:                          # the tail alone: u and g would not be read
            draws = (None, None, torch.rand([n, N_UNIFORM_TAIL], device=images.device), torch.randn([n, N_NORMAL_TAIL], device=images.device))
        draws = tuple(draws)
        if len(draws) not in ((4, 5) if tail else (2, 4, 5)):
            raise ValueError(f'FullAugmentPipe: draws must be (u, g, ut, gt) or (u, g, ut, gt, z){"" if tail else " or (u, g)"} '
                             f'(got {len(draws)} entries)')
        images = super().forward(images, draws[:2])
        if not tail:
            return images
        Hz, sigma, cut = self.tail_params(draws)
        z = None
        if self.noise > 0:
            z = draws[4] if len(draws) == 5 else torch.randn([n, color[1], h, w], device=images.device)
        return ada_tail_apply(images, Hz if self.imgfilter > 0 else None, sigma if z is not None else None, z,
                              cut if self.cutout > 0 else None, color)
