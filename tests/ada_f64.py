"""The yardstick of the ADA pipe tests: StyleGAN2-ADA's ``AugmentPipe.forward`` (blit, geometry, colour) restated literally with torch's
own operators on the CPU, in the dtype asked for -- ``F.pad(reflect)``, zero insertion + ``conv2d`` for the two FIR passes,
``F.affine_grid`` + ``F.grid_sample`` -- with the draws passed in (column layout of ``shgan_amd.ada``).  Shares no code with the package."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SYM6 = [0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633, 0.4910559419267466, 0.787641141030194,
        0.3379294217276218, -0.07263752278646252, -0.021060292512300564, 0.04472490177066578, 0.0017677118642428036, -0.007800708325034148]

DEFAULTS = dict(xflip=0, rotate90=0, xint=0, xint_max=0.125, scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2,
                xfrac_std=0.125, brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1,
                saturation_std=1)
GEOM_KEYS = ('xflip', 'rotate90', 'xint', 'scale', 'rotate', 'aniso', 'xfrac')
COLOR_KEYS = ('brightness', 'contrast', 'lumaflip', 'hue', 'saturation')


def hz_geom(dtype):
    f = torch.tensor(SYM6, dtype=torch.float64)
    return (f / f.sum()).to(dtype)


# ---- ADA's matrix helpers -------------------------------------------------------------------------------------------------------------
def matrix(*rows, dtype):
    """rows of scalars / [N] tensors -> [N, r, c] (or [r, c] when everything is a scalar)."""
    elems = [x for row in rows for x in row]
    ref = [x for x in elems if isinstance(x, torch.Tensor)]
    if not ref:
        return torch.tensor(rows, dtype=dtype)
    elems = [x if isinstance(x, torch.Tensor) else torch.full(ref[0].shape, float(x), dtype=dtype) for x in elems]
    return torch.stack(elems, dim=-1).reshape(ref[0].shape + (len(rows), -1))


def translate2d(tx, ty, dtype):
    return matrix([1, 0, tx], [0, 1, ty], [0, 0, 1], dtype=dtype)


def translate3d(tx, ty, tz, dtype):
    return matrix([1, 0, 0, tx], [0, 1, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1], dtype=dtype)


def scale2d(sx, sy, dtype):
    return matrix([sx, 0, 0], [0, sy, 0], [0, 0, 1], dtype=dtype)


def scale3d(sx, sy, sz, dtype):
    return matrix([sx, 0, 0, 0], [0, sy, 0, 0], [0, 0, sz, 0], [0, 0, 0, 1], dtype=dtype)


def rotate2d(theta, dtype):
    if not isinstance(theta, torch.Tensor):
        theta = torch.tensor(theta, dtype=dtype)
    return matrix([torch.cos(theta), torch.sin(-theta), 0], [torch.sin(theta), torch.cos(theta), 0], [0, 0, 1], dtype=dtype)


def rotate3d(v, theta, dtype):
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    s, c = torch.sin(theta), torch.cos(theta)
    cc = 1 - c
    return matrix([vx * vx * cc + c, vx * vy * cc - vz * s, vx * vz * cc + vy * s, 0], [vy * vx * cc + vz * s, vy * vy * cc + c, vy * vz * cc - vx * s, 0],
                  [vz * vx * cc - vy * s, vz * vy * cc + vx * s, vz * vz * cc + c, 0], [0, 0, 0, 1], dtype=dtype)


def translate2d_inv(tx, ty, dtype):
    return translate2d(-tx, -ty, dtype)


def scale2d_inv(sx, sy, dtype):
    return scale2d(1 / sx, 1 / sy, dtype)


def rotate2d_inv(theta, dtype):
    return rotate2d(-theta, dtype)


# ---- parameters from draws ------------------------------------------------------------------------------------------------------------
def params(u, g, p, cfg, H, W, dtype, color_count=3):
    """-> dict(G_inv [N,3,3], C [N,3,4], xint_pre [N,2]: the products ``t * size`` before ``round``)."""
    k = dict(DEFAULTS)
    k.update(cfg)
    u, g = u.to(dtype), g.to(dtype)
    p = torch.as_tensor(p, dtype=torch.float32).to(dtype)
    N = u.shape[0]
    I_3 = torch.eye(3, dtype=dtype)
    G_inv = I_3
    zeros, ones = torch.zeros([N], dtype=dtype), torch.ones([N], dtype=dtype)
    xint_pre = torch.zeros([N, 2], dtype=dtype)
    if k['xflip'] > 0:
        i = torch.floor(u[:, 0] * 2)
        i = torch.where(u[:, 1] < k['xflip'] * p, i, zeros)
        G_inv = G_inv @ scale2d_inv(1 - 2 * i, 1, dtype)
    if k['rotate90'] > 0:
        i = torch.floor(u[:, 2] * 4)
        i = torch.where(u[:, 3] < k['rotate90'] * p, i, zeros)
        G_inv = G_inv @ rotate2d_inv(-np.pi / 2 * i, dtype)
    if k['xint'] > 0:
        t = (u[:, 4:6] * 2 - 1) * k['xint_max']
        t = torch.where((u[:, 6] < k['xint'] * p).unsqueeze(1), t, torch.zeros_like(t))
        xint_pre = torch.stack([t[:, 0] * W, t[:, 1] * H], dim=1)
        G_inv = G_inv @ translate2d_inv(torch.round(t[:, 0] * W), torch.round(t[:, 1] * H), dtype)
    if k['scale'] > 0:
        s = torch.exp2(g[:, 0] * k['scale_std'])
        s = torch.where(u[:, 7] < k['scale'] * p, s, ones)
        G_inv = G_inv @ scale2d_inv(s, s, dtype)
    p_rot = 1 - torch.sqrt((1 - k['rotate'] * p).clamp(0, 1))
    if k['rotate'] > 0:
        theta = (u[:, 8] * 2 - 1) * np.pi * k['rotate_max']
        theta = torch.where(u[:, 9] < p_rot, theta, zeros)
        G_inv = G_inv @ rotate2d_inv(-theta, dtype)
    if k['aniso'] > 0:
        s = torch.exp2(g[:, 1] * k['aniso_std'])
        s = torch.where(u[:, 10] < k['aniso'] * p, s, ones)
        G_inv = G_inv @ scale2d_inv(s, 1 / s, dtype)
    if k['rotate'] > 0:
        theta = (u[:, 11] * 2 - 1) * np.pi * k['rotate_max']
        theta = torch.where(u[:, 12] < p_rot, theta, zeros)
        G_inv = G_inv @ rotate2d_inv(-theta, dtype)
    if k['xfrac'] > 0:
        t = g[:, 2:4] * k['xfrac_std']
        t = torch.where((u[:, 13] < k['xfrac'] * p).unsqueeze(1), t, torch.zeros_like(t))
        G_inv = G_inv @ translate2d_inv(t[:, 0] * W, t[:, 1] * H, dtype)
    G_inv = G_inv.expand(N, 3, 3).clone() if G_inv.ndim == 2 else G_inv

    I_4 = torch.eye(4, dtype=dtype)
    C = I_4
    if k['brightness'] > 0:
        b = g[:, 4] * k['brightness_std']
        b = torch.where(u[:, 14] < k['brightness'] * p, b, zeros)
        C = translate3d(b, b, b, dtype) @ C
    if k['contrast'] > 0:
        c = torch.exp2(g[:, 5] * k['contrast_std'])
        c = torch.where(u[:, 15] < k['contrast'] * p, c, ones)
        C = scale3d(c, c, c, dtype) @ C
    v = torch.tensor([1, 1, 1, 0], dtype=dtype) / np.sqrt(3)
    if k['lumaflip'] > 0:
        i = torch.floor(u[:, 16].reshape(N, 1, 1) * 2)
        i = torch.where(u[:, 17].reshape(N, 1, 1) < k['lumaflip'] * p, i, torch.zeros_like(i))
        C = (I_4 - 2 * v.ger(v) * i) @ C
    if k['hue'] > 0 and color_count > 1:
        theta = (u[:, 18] * 2 - 1) * np.pi * k['hue_max']
        theta = torch.where(u[:, 19] < k['hue'] * p, theta, zeros)
        C = rotate3d(v, theta, dtype) @ C
    if k['saturation'] > 0 and color_count > 1:
        s = torch.exp2(g[:, 6].reshape(N, 1, 1) * k['saturation_std'])
        s = torch.where(u[:, 20].reshape(N, 1, 1) < k['saturation'] * p, s, torch.ones_like(s))
        C = (v.ger(v) + (I_4 - v.ger(v)) * s) @ C
    C = C.expand(N, 4, 4).clone() if C.ndim == 2 else C
    return dict(G_inv=G_inv, C=C[:, :3, :].contiguous(), xint_pre=xint_pre)


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def margins_pre(G_inv, H, W):
    """ADA's margin before ``ceil`` ([4] = x0, y0, x1, y1, clamped), in G_inv's dtype."""
    dtype = G_inv.dtype
    cx, cy = (W - 1) / 2, (H - 1) / 2
    cp = matrix([-cx, -cy, 1], [cx, -cy, 1], [cx, cy, 1], [-cx, cy, 1], dtype=dtype)
    cp = G_inv @ cp.t()
    Hz_pad = len(SYM6) // 4
    margin = cp[:, :2, :].permute(1, 0, 2).flatten(1)
    margin = torch.cat([-margin, margin]).max(dim=1).values
    margin = margin + torch.tensor([Hz_pad * 2 - cx, Hz_pad * 2 - cy] * 2, dtype=dtype)
    margin = margin.max(torch.tensor([0, 0] * 2, dtype=dtype))
    margin = margin.min(torch.tensor([W - 1, H - 1] * 2, dtype=dtype))
    return margin


def _fir(x, f, axis):
    C = x.shape[1]
    w = f.reshape(1, 1, -1, 1) if axis == 2 else f.reshape(1, 1, 1, -1)
    return F.conv2d(x, w.repeat(C, 1, 1, 1), groups=C)


def upsample2d(x, f):
    """upfirdn2d.upsample2d(x, f, up=2): zero insertion, padding (6, 5) per axis, true convolution, gain 4."""
    N, C, H, W = x.shape
    z = x.reshape(N, C, H, 1, W, 1)
    z = F.pad(z, [0, 1, 0, 0, 0, 1])
    z = z.reshape(N, C, H * 2, W * 2)
    z = F.pad(z, [6, 5, 6, 5])
    ff = (f * 2).flip(0)                       # gain ** (ndim / 2) per axis; not flip_filter -> flipped for conv2d (a correlation)
    return _fir(_fir(z, ff, 2), ff, 3)


def downsample2d(x, f):
    """upfirdn2d.downsample2d(x, f, down=2, padding=-6, flip_filter=True): padding (-1, -1) per axis, correlation, every second sample."""
    x = x[:, :, 1:-1, 1:-1]
    x = _fir(_fir(x, f, 2), f, 3)
    return x[:, :, ::2, ::2]


def geometry(x, G_inv, margins=None, samples=None):
    """ADA's geometric execution on given matrices -> (y, (mx0, my0, mx1, my1)).  ``margins``: use these integers instead of ``ceil`` of
    this dtype's own (a float32 run next to a float64 one: no integer decision is in play).  ``samples``: a list that receives the output
    of ``grid_sample`` (the x2 sample grid before the decimating filter)."""
    dtype = x.dtype
    G_inv = G_inv.to(dtype)
    N, C, H, W = x.shape
    f = hz_geom(dtype)
    Hz_pad = len(SYM6) // 4
    if margins is None:
        margins = [int(v) for v in margins_pre(G_inv, H, W).ceil().to(torch.int32)]
    mx0, my0, mx1, my1 = margins
    x = F.pad(x, [mx0, mx1, my0, my1], mode='reflect')
    G_inv = translate2d((mx0 - mx1) / 2, (my0 - my1) / 2, dtype) @ G_inv
    x = upsample2d(x, f)
    G_inv = scale2d(2, 2, dtype) @ G_inv @ scale2d_inv(2, 2, dtype)
    G_inv = translate2d(-0.5, -0.5, dtype) @ G_inv @ translate2d_inv(-0.5, -0.5, dtype)
    shape = [N, C, (H + Hz_pad * 2) * 2, (W + Hz_pad * 2) * 2]
    G_inv = scale2d(2 / x.shape[3], 2 / x.shape[2], dtype) @ G_inv @ scale2d_inv(2 / shape[3], 2 / shape[2], dtype)
    grid = F.affine_grid(theta=G_inv[:, :2, :], size=shape, align_corners=False)
    x = F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    if samples is not None:
        samples.append(x)
    x = downsample2d(x, f)
    return x, tuple(margins)


# ---- colour ---------------------------------------------------------------------------------------------------------------------------
def color(x, C34, channels, bias=True):
    """ADA's colour execution on channels (first, count) of x with the [N,3,4] matrix; the other channels pass."""
    first, count = channels
    dtype = x.dtype
    C34 = C34.to(dtype)
    N, _, H, W = x.shape
    img = x[:, first:first + count].reshape(N, count, H * W)
    t = C34[:, :, 3:] if bias else torch.zeros_like(C34[:, :, 3:])
    if count == 3:
        img = C34[:, :3, :3] @ img + t
    else:
        Cm = C34.mean(dim=1, keepdims=True)
        img = img * Cm[:, :, :3].sum(dim=2, keepdims=True) + t.mean(dim=1, keepdims=True)
    return torch.cat([x[:, :first], img.reshape(N, count, H, W), x[:, first + count:]], dim=1)


# ---- the whole pipe ---------------------------------------------------------------------------------------------------------------------
def pipe(x, u, g, p, cfg, channels, margins=None):
    k = dict(DEFAULTS)
    k.update(cfg)
    pr = params(u, g, p, cfg, x.shape[2], x.shape[3], x.dtype, color_count=channels[1])
    m = None
    if any(k[n] > 0 for n in GEOM_KEYS):
        x, m = geometry(x, pr['G_inv'], margins)
    if any(k[n] > 0 for n in COLOR_KEYS):
        x = color(x, pr['C'], channels)
    return x, m


def apply(x, G_inv=None, C34=None, channels=None, margins=None, bias=True):
    """geometry (when G_inv is given) then colour (when C34 is) in x's dtype."""
    if G_inv is not None:
        x, _ = geometry(x, G_inv, margins)
    if C34 is not None:
        x = color(x, C34, channels, bias=bias)
    return x


def adjoint(w, x_shape, G_inv=None, C34=None, channels=None, margins=None):
    """A^T w by autograd of ``apply`` in w's dtype."""
    with torch.enable_grad():
        x = torch.zeros(x_shape, dtype=w.dtype, requires_grad=True)
        y = apply(x, G_inv, C34, channels, margins, bias=False)
        (gx,) = torch.autograd.grad((y * w).sum(), x)
    return gx.detach()


def second_order_wgrad(w, x_shape, G_inv=None, C34=None, channels=None, margins=None):
    """d/dw |A^T w|^2 = 2 A A^T w.  ``grid_sampler_2d_backward`` has no derivative in torch (the reason ADA ships ``grid_sample_gradfix``),
    so the double backward of the restatement is spelled out with its own first-order autograd: A^T w by ``adjoint``, then A on it."""
    gx = adjoint(w, x_shape, G_inv, C34, channels, margins)
    return 2 * apply(gx, G_inv, C34, channels, margins, bias=False)


def affine(kind, N, H, W, dtype=torch.float64):
    """The named G_inv matrices of the apply tests (ADA's convention), [N,3,3]."""
    eye = torch.eye(3, dtype=dtype).expand(N, 3, 3).clone()
    if kind == 'identity':
        return eye
    if kind == 'shift':
        return translate2d(3.0, -2.0, dtype).expand(N, 3, 3).clone()
    if kind == 'rot_aniso_frac':
        m = rotate2d_inv(-0.4, dtype) @ scale2d_inv(1.3, 1 / 1.3, dtype) @ translate2d_inv(0.37 * 3, -0.21 * 5, dtype)
        return m.expand(N, 3, 3).clone()
    if kind == 'zoom_out4':
        return scale2d(4.0, 4.0, dtype).expand(N, 3, 3).clone()
    if kind == 'zoom_in2':
        return scale2d(0.5, 0.5, dtype).expand(N, 3, 3).clone()
    if kind == 'xflip':
        return scale2d_inv(-1.0, 1.0, dtype).expand(N, 3, 3).clone()
    if kind == 'rot90':
        return rotate2d_inv(-math.pi / 2, dtype).expand(N, 3, 3).clone()
    if kind == 'mixed':
        m = eye
        m[N - 1] = scale2d(1.6, 1.6, dtype)
        return m
    raise KeyError(kind)


AFFINE_KINDS = ('identity', 'shift', 'rot_aniso_frac', 'zoom_out4', 'zoom_in2', 'xflip', 'rot90', 'mixed')
