"""Test helper: the float64 yardstick of ``Lpips.loss`` and of its gradient with respect to the pred image, by float64 autograd through
the models of tests/lpips_f64.py (AlexNet, random weights) and tests/ppl_f64.py (VGG16 at the ``NARROW`` widths, random weights).  Both
operands are float32 images in [-1, 1] that enter the scaling layer as they are.  The normaliser is written
``ss.clamp_min(1e-300).sqrt() + 1e-10`` so that a position whose tap vector is all zero gives finite values, which the ReLU backward then
zeroes -- the convention the HIP head implements with a select.

Every case must meet two conditions, ASSERTED on the float64 run by ``check_conditions``:
 (a) at least one position of some pred tap has an all-zero vector (the select path is exercised);
 (b) no pool window attains a positive maximum twice (the tie rule of the pool backward is then immaterial to the gradient).
The same functions run in float32 (``dtype=torch.float32``) are torch's own CPU autograd of the same model: the ``e_ref`` of the bar
``max(LAYER_FACTOR * e_ref, LAYER_FLOOR)`` of tests/second_order_f64.py.  Nothing here is shipped."""
import torch
import torch.nn.functional as F

import lpips_f64
import ppl_f64
from second_order_f64 import LAYER_FACTOR, LAYER_FLOOR

NARROW = ppl_f64.NARROW
# (net, B, H, W) of the end-to-end cases.  vgg 16 x 16: the minimum, the last tap is 1 x 1 and the convolution tiles are partial; 35 x 37:
# odd at three pool levels.  alex 31 x 31: the minimum; 33 x 46: the last column lies in no conv1 window, the pools give 2 and 1 outputs;
# 67 x 35.  Seeds for which conditions (a) and (b) hold in every case, found by a scan on the CPU.
CASES = (('vgg', 1, 16, 16), ('vgg', 3, 16, 16), ('vgg', 1, 35, 37), ('vgg', 3, 35, 37), ('alex', 3, 31, 31), ('alex', 1, 33, 46), ('alex', 3, 33, 46),
         ('alex', 3, 67, 35))
WEIGHT_SEED, IMAGE_SEED = 1, 0


def state_dict(net, seed):
    """'vgg': ``ppl_f64.vgg_random_state_dict(NARROW, seed)``.  'alex': ``lpips_f64.random_state_dict(seed)`` with the first convolution's
    biases made negative, so that a flat patch of the shift colour (scaled value exactly 0) gives an all-zero tap-0 vector: at 64+ channels
    condition (a) does not happen by chance."""
    if net == 'vgg':
        return ppl_f64.vgg_random_state_dict(NARROW, seed)
    sd = lpips_f64.random_state_dict(seed)
    sd['net.slice1.0.bias'] = -sd['net.slice1.0.bias'].abs() - 0.01
    return sd


def images(net, B, H, W, seed):
    """(fake, real) float32 [B,3,H,W] in [-1, 1].  'alex': ``fake`` carries a flat patch of the shift colour (see ``state_dict``)."""
    g = torch.Generator().manual_seed(int(seed))
    real = torch.rand(B, 3, H, W, generator=g) * 1.8 - 0.9
    fake = (real + 0.3 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)
    if net == 'alex':
        shift = torch.tensor(lpips_f64.SHIFT, dtype=torch.float32).reshape(1, 3, 1, 1)
        fake[:, :, 4:23, 4:23] = shift
    return fake.contiguous(), real.contiguous()


def upstream(B):
    """A distinct upstream gradient per sample, one of them 0 (that sample's image gradient must be exact zeros)."""
    return torch.tensor([0.75, 0.0, -1.5, 0.3125, 2.0][:B], dtype=torch.float32)


def scaling(v, dtype):
    sh = torch.tensor(lpips_f64.SHIFT, dtype=torch.float32).to(dtype)[None, :, None, None]
    sc = torch.tensor(lpips_f64.SCALE, dtype=torch.float32).to(dtype)[None, :, None, None]
    return (v.to(dtype) - sh) / sc


def trunk(net, sd, x, dtype, pooled=None):
    """Scaled input -> the five taps in ``dtype``; ``pooled``: a list that receives (pool input, window) of every max pool."""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    if net == 'vgg':
        taps = []
        for k, (s, i) in enumerate(zip(ppl_f64.VGG_SLICE_OF, ppl_f64.VGG_CONV_IDS)):
            key = f'net.slice{s}.{i}'
            x = F.relu(F.conv2d(x, sdd[f'{key}.weight'], sdd[f'{key}.bias'], padding=1))
            if k in ppl_f64.VGG_TAPS:
                taps.append(x)
                if k != ppl_f64.VGG_TAPS[-1]:
                    if pooled is not None:
                        pooled.append((x, 2))
                    x = F.max_pool2d(x, 2, 2)
        return taps
    taps = []
    for n, (key, _, _, _, s, p) in enumerate(lpips_f64.CONVS):
        if n in (1, 2):
            if pooled is not None:
                pooled.append((x, 3))
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sdd[f'{key}.weight'], sdd[f'{key}.bias'], stride=s, padding=p))
        taps.append(x)
    return taps


def head(f, fr, w):
    """One tap -> [B]: the spatial mean of sum_c w_c (f^ - fr^)^2, f^ = f / (sqrt(sum f^2) + 1e-10); finite gradients at sum f^2 = 0."""
    w = w.to(f.dtype).reshape(1, -1, 1, 1)
    n0 = f / ((f ** 2).sum(dim=1, keepdim=True).clamp_min(1e-300).sqrt() + 1e-10)
    n1 = fr / ((fr ** 2).sum(dim=1, keepdim=True).clamp_min(1e-300).sqrt() + 1e-10)
    return (w * (n0 - n1) ** 2).sum(dim=1).mean(dim=(1, 2))


def loss(net, sd, fake, real, dtype=torch.float64, pooled=None):
    """float32 images in [-1, 1] -> [B] in ``dtype`` (differentiable with respect to ``fake``)."""
    tp = trunk(net, sd, scaling(fake, dtype), dtype, pooled)
    with torch.no_grad():
        tr = trunk(net, sd, scaling(real, dtype), dtype)
    return sum(head(a, b, sd[f'lin{n}.model.1.weight']) for n, (a, b) in enumerate(zip(tp, tr))), tp


def loss_and_grad(net, sd, fake, real, g, dtype=torch.float64, conditions=False):
    """-> (loss [B], d(sum_b g_b loss_b) / d fake) on the CPU in ``dtype``.  ``conditions``: assert (a) and (b) on this run."""
    with torch.enable_grad():
        x = fake.detach().clone().to(dtype).requires_grad_(True)
        pooled = [] if conditions else None
        value, taps = loss(net, sd, x, real, dtype, pooled)
        (grad,) = torch.autograd.grad((value * g.to(dtype)).sum(), x)
    if conditions:
        check_conditions(taps, pooled)
    return value.detach(), grad


def check_conditions(taps, pooled):
    dead = sum(int(((t.detach() ** 2).sum(dim=1) == 0).sum()) for t in taps)
    assert dead > 0, '(a) no pred tap has an all-zero vector at any position: the select path is not exercised'
    for x, k in pooled:
        x = x.detach()
        win = F.unfold(x.reshape(-1, 1, *x.shape[2:]), k, stride=2)              # [BC, k*k, L]
        top = win.max(dim=1, keepdim=True).values
        twice = ((win == top).sum(dim=1, keepdim=True) > 1) & (top > 0)
        assert not bool(twice.any()), '(b) a pool window attains a positive maximum twice'


def rel_inf(x, x64):
    """||x - x64||_inf / ||x64||_inf of one tensor."""
    x64 = x64.detach().cpu().to(torch.float64)
    return float((x.detach().cpu().to(torch.float64) - x64).abs().max() / x64.abs().max().clamp_min(1e-300))


def bar(e_ref):
    return max(LAYER_FACTOR * e_ref, LAYER_FLOOR)


# ---- the operators on their own -------------------------------------------------------------------------------------------------------

def head_grad_closed_form(f, fr, w, g):
    """The formula csrc/lpips_bwd.hip implements, in the operands' dtype: df_c = a q_c - f_c a^2 (sum_j q_j f_j) / s selected by f_c > 0."""
    B, C, h, wd = f.shape
    w = w.to(f.dtype).reshape(1, -1, 1, 1)
    s = (f ** 2).sum(dim=1, keepdim=True).sqrt()
    a = 1 / (s + 1e-10)
    nr = fr / ((fr ** 2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
    q = 2 * w * (a * f - nr) * g.to(f.dtype).reshape(-1, 1, 1, 1) / (h * wd)
    dot = (q * f).sum(dim=1, keepdim=True)
    t = torch.where(s > 0, a * a * dot / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    return torch.where(f > 0, a * q - f * t, torch.zeros_like(f))


def head_grad_autograd(f, fr, w, g):
    """Autograd through relu -> head: f = relu(z) with z = f where f > 0 and z = -1 elsewhere, so the ReLU backward zeroes what the select does."""
    with torch.enable_grad():
        z = torch.where(f > 0, f, -torch.ones_like(f)).detach().requires_grad_(True)
        (gz,) = torch.autograd.grad((head(F.relu(z), fr, w) * g.to(f.dtype)).sum(), z)
    return gz


def pool_grad_gather(x, gy, k):
    """The gather rule of the pool backward in plain loops: each input element sums the gradients of the windows whose FIRST maximum in
    row-major order it is; then the x > 0 select."""
    B, C, H, W = x.shape
    OH, OW = (H - k) // 2 + 1, (W - k) // 2 + 1
    dx = torch.zeros_like(x)
    xs = x.reshape(B * C, H, W)
    for oy in range(OH):
        for ox in range(OW):
            win = xs[:, 2 * oy:2 * oy + k, 2 * ox:2 * ox + k].reshape(B * C, -1)
            idx = first_argmax(win)
            dy, dxx = idx // k, idx % k
            dx.reshape(B * C, H, W)[torch.arange(B * C), 2 * oy + dy, 2 * ox + dxx] += gy.reshape(B * C, OH, OW)[:, oy, ox]
    return torch.where(x > 0, dx, torch.zeros_like(dx))


def first_argmax(win):
    top = win.max(dim=1, keepdim=True).values
    pos = torch.arange(win.shape[1]).expand_as(win)
    return torch.where(win == top, pos, torch.full_like(pos, win.shape[1])).min(dim=1).values


def pool_grad_autograd(x, gy, k):
    """``F.max_pool2d``'s backward on the CPU, then the x > 0 select."""
    with torch.enable_grad():
        z = x.detach().clone().requires_grad_(True)
        (dx,) = torch.autograd.grad(F.max_pool2d(z, k, 2), z, gy)
    return torch.where(x > 0, dx, torch.zeros_like(dx))


def conv_input_grad_autograd(g, w, x_shape, stride, pad):
    with torch.enable_grad():
        x = torch.zeros(x_shape, dtype=g.dtype).requires_grad_(True)
        (dx,) = torch.autograd.grad(F.conv2d(x, w, stride=stride, padding=pad), x, g)
    return dx
