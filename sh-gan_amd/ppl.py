"""Perceptual path length -- ``metric_main.py``'s ``ppl2_wend`` (the reference's lib/evaluator/stylegan_metrics/perceptual_path_length.py)
-- for the plain StyleGAN2 ``Generator`` (model_zoo/stylegan.py: ``Mapping`` + ``Synthesis``), end to end on the device.

    vgg = lpips.LPIPS(net='vgg', state_dict=sd, device='cuda')           # + mean=, std=, bgr=: the path-length detector's constants
    value = ppl.ppl2_wend(G, vgg)                                        # float; compute_ppl(G, vgg, num_samples=50000, ...)
    dist = ppl.PPLSampler(G, vgg)(torch.zeros(2, 0, device='cuda'))      # float64 [B] on the device

One ``sampler(c)`` call takes the reference's draws in the reference's order (:50-66): ``t = rand([B])`` (times 0 for 'end'),
``randn([2B, z_dim])`` chunked into z0, z1, then for 'w' one ``G.mapping`` call on the concatenation and ``w0.lerp(w1, t)``,
``w0.lerp(w1, t + epsilon)`` -- for 'z' ``slerp`` (:22-31) and then the mapping --, then one ``randn`` per ``*.noise_const`` buffer in
``named_buffers()`` order, written into a deep copy of ``G`` made at construction (the caller's generator is never modified).  Then one
``G.synthesis(ws=cat, noise_mode='const', force_fp32=True)`` under ``no_grad``, one front-end launch (``frontend``: csrc/ppl.hip -- crop,
box downsample to 256, [-1, 1] -> [0, 255], grey -> RGB, the detector's normalisation, in one pass where the reference makes four), the
VGG16 trunk of ``lpips.Lpips(net='vgg')`` once on all 2B images, and the five distance-head launches with the first half against the
second into one float64 [B] accumulator; ``dist = acc / epsilon**2`` in float64.  The LPIPS vector the reference's ``vgg16.pt`` returns
(8 M floats per image at 256 x 256) is never formed: the head reduces each tap where it lies.

All draws come from the given ``torch.Generator`` on the device (default: the device's own).  The reference draws from CUDA's global
generator; bit equality with its draws is NOT claimed: the same distribution in the same order, not the same numbers.

NOT verified here (``vgg16.pt`` is a download and is not shipped): that the detector normalises a 0..255 image with the caffe-style mean
(123.68, 116.779, 103.939) and unit std in RGB order -- the defaults ``vgg16.Vgg16Features`` uses, which is why ``mean``, ``std`` and
``bgr`` are options of the ``lpips.LPIPS(net='vgg')`` constructor --; that its ``lin`` weights are those of the ``lpips`` package's
``vgg.pth`` (their source is a constructor option too: ``lin_state_dict=``); and that it applies no LPIPS scaling layer on this route
(none is applied here).  The draw order, the interpolation, the front end's arithmetic and the trimmed mean restate the reference's
Python source, which is present, and are pinned on float64 restatements (tests/ppl_f64.py).

``compute_ppl`` runs the sampling loop of :106-119 on every rank and, for ``world > 1``, makes ONE all-gather of the ``[n]`` float64
distances at the end (``evaluators.Collective``) instead of a broadcast per batch and rank; the gathered values are interleaved in the
reference's order (batch-major, then rank) and cut to ``num_samples``.  Every rank returns the value (the reference returns NaN on ranks
other than 0).  ``trimmed_mean`` is the tail :124-127 on the device."""
import copy

import torch

from . import _lib, kernels
from ._lib import ShgError, check

INPAINTER_REASON = ('the path length walks the latent space of a generator with the image free to change everywhere; a co-modulated '
                    'inpainter (shgan_*, comodgan_*) is conditioned on the known pixels, which a latent step does not move, so the path '
                    'length says nothing about it')


def frontend_side(C, H, W, factor, crop):
    """Side S of the front end's output for an x [N,C,H,W], or None where the kernel refuses the geometry."""
    if C not in (1, 3) or H != W or H < 1 or not 0 <= int(factor) <= 256:
        return None
    side, f = (4 * (H // 8) if crop else H), max(int(factor), 1)
    return side // f if side >= 1 and side % f == 0 else None


def frontend(images, factor, crop=False, mean=(123.68, 116.779, 103.939), std=(1.0, 1.0, 1.0), y=None):
    """images [N,C,R,R] float32 in [-1, 1], C in {1, 3} -> [N,3,S,S] float32 (one launch): centre crop ``[c*3:c*7, c*2:c*6]``, c = R // 8,
    when ``crop``; mean over ``factor x factor`` boxes (``factor = img_resolution // 256``; 0 and 1 copy); ``(v + 1) * (255 / 2)``;
    a single channel repeated to three; ``(v - mean_c) / std_c``.  A non-contiguous view is copied first, as for every operand of this
    library.  A geometry the kernel refuses (non-square, C not 1 or 3, a side the factor does not divide) raises ShgError with its
    message and writes nothing; ``y``: a contiguous float32 [N,3,S,S] tensor to write into."""
    if not isinstance(images, torch.Tensor) or images.ndim != 4:
        raise ShgError('ppl: images must be a [N,C,R,R] tensor')
    L = kernels._Launch()
    x = L.req(images, 'images')
    N, C, H, W = x.shape
    S = frontend_side(C, H, W, factor, crop)
    if y is None:
        y = L.new((N, 3, S, S) if S is not None else (1,))
    else:
        L.req(y, 'y')
        if not y.is_contiguous() or (S is not None and tuple(y.shape) != (N, 3, S, S)):
            raise ShgError(f'ppl: y must be a contiguous float32 {(N, 3, S, S)} tensor (got {tuple(y.shape)})')
    with L:
        check(_lib.get_lib().shg_ppl_frontend_f32(kernels._ptr(x), kernels._ptr(y), N, C, H, W, int(factor), int(bool(crop)), kernels._c3(mean),
                                                  kernels._c3(std), L.stream()), 'ppl_frontend')
    return y


def slerp(a, b, t):
    """Spherical interpolation of a batch of vectors (:22-31)."""
    a = a / a.norm(dim=-1, keepdim=True)
    b = b / b.norm(dim=-1, keepdim=True)
    d = (a * b).sum(dim=-1, keepdim=True)
    p = t * torch.acos(d)
    c = b - d * a
    c = c / c.norm(dim=-1, keepdim=True)
    d = a * torch.cos(p) + c * torch.sin(p)
    return d / d.norm(dim=-1, keepdim=True)


def path_distance(vgg, img, factor, crop=False):
    """img [2B,C,R,R] (the synthesis output of the B path points and their B neighbours) -> float64 [B]: the squared LPIPS-VGG distance
    of image b and image B + b.  One front-end launch, the trunk once on all 2B images, five head launches into one accumulator."""
    from . import lpips
    if img.shape[0] % 2:
        raise ShgError(f'ppl: the batch of {img.shape[0]} images is not two halves')
    B = img.shape[0] // 2
    x = frontend(img, factor, crop, vgg.mean, vgg.std)
    acc = torch.zeros(B, dtype=torch.float64, device=x.device)
    for t, w in zip(vgg.trunk(x), vgg.lins):
        lpips.head(t[:B], t[B:], w, acc)
    return acc


class PPLSampler:
    """``sampler(c) -> dist`` float64 [B] on c's device (c: [B, 0]).  ``vgg``: ``lpips.LPIPS(net='vgg', ...)``, or any callable
    ``vgg(img, factor=..., crop=...) -> float64 [B]`` of ``path_distance``'s form (CPU tests).  See the module docstring."""

    def __init__(self, G, vgg, epsilon=1e-4, space='w', sampling='end', crop=False, G_kwargs=None, generator=None):
        if space not in ('z', 'w') or sampling not in ('full', 'end'):
            raise ShgError(f"ppl: space must be 'z' or 'w' and sampling 'full' or 'end' (got {space!r}, {sampling!r})")
        if not (hasattr(G, 'mapping') and hasattr(G, 'synthesis')):
            raise ShgError(f'ppl: {type(G).__name__} has no .mapping / .synthesis: the path length needs a plain generator')
        if hasattr(G, 'encoder'):              # the co-modulated generators derive from the plain one: the encoder tells them apart
            raise ShgError(f'ppl: {type(G).__name__} is an inpainting generator: {INPAINTER_REASON}')
        if int(getattr(G, 'c_dim', 0)) > 0:
            raise NotImplementedError('ppl: label-conditioned generators (c_dim > 0) are not on this path')
        if hasattr(vgg, 'trunk'):
            if getattr(vgg, 'net', None) != 'vgg':
                raise ShgError("ppl: the detector must be lpips.LPIPS(net='vgg', ...)")
            self.distance_fn = lambda img, factor, crop: path_distance(vgg, img, factor, crop)
        elif callable(vgg):
            self.distance_fn = lambda img, factor, crop: vgg(img, factor=factor, crop=crop)
        else:
            raise ShgError("ppl: vgg must be lpips.LPIPS(net='vgg', ...) or a callable vgg(img, factor=..., crop=...)")
        self.G = copy.deepcopy(G).eval().requires_grad_(False)
        self.G_kwargs = dict(G_kwargs or {})
        self.epsilon, self.space, self.sampling, self.crop, self.generator = float(epsilon), space, sampling, bool(crop), generator

    def draw(self, B, device):
        """The latent draws of one call, in the reference's order -> (t [B], z0, z1 [B, z_dim])."""
        t = torch.rand([B], device=device, generator=self.generator) * (1 if self.sampling == 'full' else 0)
        z0, z1 = torch.randn([B * 2, self.G.z_dim], device=device, generator=self.generator).chunk(2)
        return t, z0, z1

    def path_ws(self, t, z0, z1, c):
        """-> (wt0, wt1): the path points and their neighbours at ``t + epsilon`` (:54-61)."""
        G, cc = self.G, torch.cat([c, c])
        if self.space == 'w':
            w0, w1 = G.mapping(z=torch.cat([z0, z1]), c=cc).chunk(2)
            tt = t.unsqueeze(1).unsqueeze(2)
            return w0.lerp(w1, tt), w0.lerp(w1, tt + self.epsilon)
        zt0 = slerp(z0, z1, t.unsqueeze(1))
        zt1 = slerp(z0, z1, t.unsqueeze(1) + self.epsilon)
        return G.mapping(z=torch.cat([zt0, zt1]), c=cc).chunk(2)

    def redraw_noise(self):
        """One ``randn`` per ``*.noise_const`` buffer of the copy, in ``named_buffers()`` order (:64-66)."""
        for name, buf in self.G.named_buffers():
            if name.endswith('.noise_const'):
                buf.copy_(torch.randn(buf.shape, device=buf.device, dtype=buf.dtype, generator=self.generator))

    def __call__(self, c):
        with torch.no_grad():
            t, z0, z1 = self.draw(c.shape[0], c.device)
            wt0, wt1 = self.path_ws(t, z0, z1, c)
            self.redraw_noise()
            img = self.G.synthesis(ws=torch.cat([wt0, wt1]), noise_mode='const', force_fp32=True, **self.G_kwargs)
            acc = self.distance_fn(img, self.G.img_resolution // 256, self.crop)
            return acc.to(torch.float64) / self.epsilon ** 2


def sampling_rounds(num_samples, batch_size, world=1):
    """Sampler calls per rank: ``len(range(0, num_samples, batch_size * world))`` (:109)."""
    return len(range(0, int(num_samples), int(batch_size) * int(world)))


def interleave(full, batch_size, num_samples):
    """full [world, rounds * batch_size] (rank r's distances in the order it drew them) -> [num_samples] in the reference's order:
    batch-major, then rank, then the position inside the batch (:114-118, :124), cut to ``num_samples``."""
    world = full.shape[0]
    return full.reshape(world, -1, int(batch_size)).permute(1, 0, 2).reshape(-1)[:int(num_samples)]


def percentile_indices(n):
    """(index of the 1st percentile with interpolation='lower', of the 99th with 'higher') in the sorted values, from numpy's definition:
    floor / ceil of q / 100 * (n - 1), in integers."""
    return (n - 1) // 100, -(-(n - 1) * 99 // 100)


def trimmed_mean(dist):
    """float64 [n] -> float: the mean of the values in [lo, hi], lo = the 1st percentile ('lower'), hi = the 99th ('higher') (:124-127).
    One sort on the values' device, ties at the bounds kept (``>=`` / ``<=``), one scalar to the host."""
    if not isinstance(dist, torch.Tensor) or dist.ndim != 1 or dist.numel() < 1:
        raise ShgError('ppl: trimmed_mean takes a non-empty 1-D tensor')
    s = torch.sort(dist.to(torch.float64)).values
    i_lo, i_hi = percentile_indices(s.numel())
    keep = (s >= s[i_lo]) & (s <= s[i_hi])
    return float(torch.where(keep, s, torch.zeros_like(s)).sum() / keep.sum())


def compute_ppl(G, vgg, num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2, rank=0, world=1, generator=None,
                collective=None):
    """The metric (:94-128) -> float.  ``generator``: this rank's ``torch.Generator`` on the device (ranks need different seeds).
    ``collective``: an ``evaluators.Collective`` (default: one over the initialised process group; CPU tests pass a stand-in)."""
    from . import evaluators
    sampler = PPLSampler(G, vgg, epsilon=epsilon, space=space, sampling=sampling, crop=crop, generator=generator)
    try:
        device = next(sampler.G.parameters()).device
    except StopIteration:
        device = torch.device('cpu')
    c = torch.zeros([int(batch_size), 0], device=device)
    rounds = sampling_rounds(num_samples, batch_size, world)
    local = torch.cat([sampler(c) for _ in range(rounds)]) if rounds else torch.zeros(0, dtype=torch.float64, device=device)
    full = local[None]
    if int(world) > 1:
        collective = collective if collective is not None else evaluators.Collective(device, rounds * int(batch_size) * int(world), world)
        full = collective.rows(local, arrange=False)            # the one collective: [world, rounds * batch_size]
    return trimmed_mean(interleave(full, batch_size, num_samples))


def ppl2_wend(G, vgg, num_samples=50000, **kw):
    """``metric_main.py``'s row: ``compute_ppl(num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2)``;
    ``kw``: rank, world, generator, collective."""
    unknown = set(kw) - {'rank', 'world', 'generator', 'collective'}
    if unknown:
        raise ShgError(f'ppl: unknown ppl2_wend option(s) {sorted(unknown)}')
    return compute_ppl(G, vgg, num_samples=num_samples, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2, **kw)
