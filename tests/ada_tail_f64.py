"""The yardstick of the ADA tail tests: the steps of StyleGAN2-ADA's ``AugmentPipe.forward`` after the colour stage -- image-space filter,
additive noise, cutout -- restated literally with numpy's and torch's own operators on the CPU, in the dtype asked for, with the draws passed
in (column layout of ``shgan_amd.ada``: ut [N,8] uniform, gt [N,5] normal).  Shares no code with the package."""
import numpy as np
import torch
import torch.nn.functional as F

SYM2 = [-0.12940952255092145, 0.22414386804185735, 0.836516303737469, 0.48296291314469025]
DEFAULTS = dict(imgfilter=0, imgfilter_bands=(1, 1, 1, 1), imgfilter_std=1, noise=0, noise_std=0.1, cutout=0, cutout_size=0.5)
TAPS, PAD = 43, 21


def hz_fbank():
    """ADA's ``Hz_fbank``, float64 [4, 43] (``scipy.signal.convolve`` of a 2-d array with a [1, 7] kernel: a per-row ``np.convolve``)."""
    Hz_lo = np.asarray(SYM2, dtype=np.float64)
    Hz_hi = Hz_lo * ((-1) ** np.arange(Hz_lo.size))
    Hz_lo2 = np.convolve(Hz_lo, Hz_lo[::-1]) / 2
    Hz_hi2 = np.convolve(Hz_hi, Hz_hi[::-1]) / 2
    fb = np.eye(4, 1)
    for i in range(1, fb.shape[0]):
        fb = np.dstack([fb, np.zeros_like(fb)]).reshape(fb.shape[0], -1)[:, :-1]
        fb = np.stack([np.convolve(row, Hz_lo2) for row in fb])
        fb[i, (fb.shape[1] - Hz_hi2.size) // 2: (fb.shape[1] + Hz_hi2.size) // 2] += Hz_hi2
    return fb


def thresholds(p, cfg):
    """The eight gate thresholds in ut's column order (bands 0..3, noise, cutout) as float64, for p as the float32 the device holds."""
    k = dict(DEFAULTS)
    k.update(cfg)
    p = float(np.float32(p))
    return [k['imgfilter'] * p * b for b in k['imgfilter_bands']] + [k['noise'] * p, k['cutout'] * p]


def params(ut, gt, p, cfg, dtype):
    """-> dict(Hz [N,43], sigma [N], cut [N,4] = cx, cy, half_w, half_h, fired [N,4] bool: the band gates)."""
    k = dict(DEFAULTS)
    k.update(cfg)
    ut, gt = ut.to(dtype), gt.to(dtype)
    p = torch.as_tensor(p, dtype=torch.float32).to(dtype)
    N = ut.shape[0]
    bank = torch.from_numpy(hz_fbank()).to(dtype)
    expected_power = (torch.tensor([10, 1, 1, 1], dtype=torch.float64) / 13).to(dtype)
    g = torch.ones([N, 4], dtype=dtype)
    fired = torch.zeros([N, 4], dtype=torch.bool)
    for i, band_strength in enumerate(k['imgfilter_bands']):
        t_i = torch.exp2(gt[:, i] * k['imgfilter_std'])
        gate = ut[:, i] < k['imgfilter'] * p * band_strength
        fired[:, i] = gate
        t_i = torch.where(gate, t_i, torch.ones_like(t_i))
        t = torch.ones([N, 4], dtype=dtype)
        t[:, i] = t_i
        t = t / (expected_power * t.square()).sum(dim=-1, keepdims=True).sqrt()
        g = g * t
    Hz = g @ bank
    sigma = gt[:, 4].abs() * k['noise_std']
    sigma = torch.where(ut[:, 4] < k['noise'] * p, sigma, torch.zeros_like(sigma))
    size = torch.full([N], float(k['cutout_size']), dtype=dtype)
    size = torch.where(ut[:, 5] < k['cutout'] * p, size, torch.zeros_like(size))
    cut = torch.stack([ut[:, 6], ut[:, 7], size / 2, size / 2], dim=1)
    return dict(Hz=Hz, sigma=sigma, cut=cut, fired=fired)


def imgfilter(x, Hz):
    """ADA's execution: reflect-pad by 21, then two grouped ``conv2d`` (along x, then along y) with each sample's taps."""
    N, C, H, W = x.shape
    Hz_prime = Hz.to(x.dtype).unsqueeze(1).repeat([1, C, 1]).reshape([N * C, 1, -1])
    p = TAPS // 2
    x = x.reshape([1, N * C, H, W])
    x = F.pad(input=x, pad=[p, p, p, p], mode='reflect')
    x = F.conv2d(input=x, weight=Hz_prime.unsqueeze(2), groups=N * C)
    x = F.conv2d(input=x, weight=Hz_prime.unsqueeze(3), groups=N * C)
    return x.reshape([N, C, H, W])


def cutout_terms(cut, H, W, dtype):
    """-> (dx [N,W], dy [N,H]): ``|coordinate - centre| - size / 2`` per axis, in the dtype asked for (the mask is ``dx >= 0 or dy >= 0``)."""
    cut = cut.to(dtype)
    coord_x = torch.arange(W, dtype=dtype).reshape(1, -1)
    coord_y = torch.arange(H, dtype=dtype).reshape(1, -1)
    dx = ((coord_x + 0.5) / W - cut[:, 0:1]).abs() - cut[:, 2:3]
    dy = ((coord_y + 0.5) / H - cut[:, 1:2]).abs() - cut[:, 3:4]
    return dx, dy


def cutout_mask(cut, H, W, dtype):
    """ADA's compares, literally: [N,1,H,W] of 0 / 1."""
    cut = cut.to(dtype)
    N = cut.shape[0]
    coord_x = torch.arange(W, dtype=dtype).reshape([1, 1, 1, -1])
    coord_y = torch.arange(H, dtype=dtype).reshape([1, 1, -1, 1])
    mask_x = (((coord_x + 0.5) / W - cut[:, 0].reshape(N, 1, 1, 1)).abs() >= cut[:, 2].reshape(N, 1, 1, 1))
    mask_y = (((coord_y + 0.5) / H - cut[:, 1].reshape(N, 1, 1, 1)).abs() >= cut[:, 3].reshape(N, 1, 1, 1))
    return torch.logical_or(mask_x, mask_y).to(dtype)


def apply(x, Hz=None, sigma=None, z=None, cut=None, channels=None, bias=True, mask_dtype=torch.float32):
    """filter (when Hz is given) and noise (sigma, z [N,count,H,W]) on channels (first, count), cutout (cut) on every channel, in x's dtype.
    The cutout compares are ADA's float32 ones whatever x's dtype: which pixels are erased is an input of the comparison, not its subject."""
    N, C, H, W = x.shape
    first, count = channels if channels is not None else (0, C)
    img = x[:, first:first + count]
    if Hz is not None:
        img = imgfilter(img, Hz)
    if sigma is not None and bias:
        img = img + z.to(x.dtype) * sigma.to(x.dtype).reshape(N, 1, 1, 1)
    x = torch.cat([x[:, :first], img, x[:, first + count:]], dim=1)
    if cut is not None:
        x = x * cutout_mask(cut, H, W, mask_dtype).to(x.dtype)
    return x


def adjoint(w, Hz=None, cut=None, channels=None):
    """A^T w by autograd of ``apply`` (its linear part) in w's dtype."""
    with torch.enable_grad():
        x = torch.zeros_like(w).requires_grad_(True)
        y = apply(x, Hz=Hz, cut=cut, channels=channels, bias=False)
        (gx,) = torch.autograd.grad((y * w).sum(), x)
    return gx.detach()


def second_order_wgrad(w, Hz=None, cut=None, channels=None):
    """d/dw |A^T w|^2 = 2 A A^T w, by autograd through autograd of the restatement."""
    with torch.enable_grad():
        wr = w.clone().requires_grad_(True)
        x = torch.zeros_like(w).requires_grad_(True)
        y = apply(x, Hz=Hz, cut=cut, channels=channels, bias=False)
        (gx,) = torch.autograd.grad((y * wr).sum(), x, create_graph=True)
        (gw,) = torch.autograd.grad(gx.square().sum(), wr)
    return gw.detach()
