"""Test helper: a float64 CPU model of the FID Inception-v3 feature extractor, written from the architecture (torchvision /
pytorch-fid ``FIDInception*`` blocks; TF1 front end of the ``inception-2015-12-05`` detector) in plain torch, and random weights from a
seed in the torchvision key layout.  Nothing here is shipped; it is the yardstick of tests/test_*inception*.py."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def _table():
    """(name, I, O, (kh, kw)) of the 94 convolutions."""
    t = [('Conv2d_1a_3x3', 3, 32, (3, 3)), ('Conv2d_2a_3x3', 32, 32, (3, 3)), ('Conv2d_2b_3x3', 32, 64, (3, 3)),
         ('Conv2d_3b_1x1', 64, 80, (1, 1)), ('Conv2d_4a_3x3', 80, 192, (3, 3))]
    for n, cin, pf in (('Mixed_5b', 192, 32), ('Mixed_5c', 256, 64), ('Mixed_5d', 288, 64)):
        t += [(f'{n}.branch1x1', cin, 64, (1, 1)), (f'{n}.branch5x5_1', cin, 48, (1, 1)), (f'{n}.branch5x5_2', 48, 64, (5, 5)),
              (f'{n}.branch3x3dbl_1', cin, 64, (1, 1)), (f'{n}.branch3x3dbl_2', 64, 96, (3, 3)), (f'{n}.branch3x3dbl_3', 96, 96, (3, 3)),
              (f'{n}.branch_pool', cin, pf, (1, 1))]
    t += [('Mixed_6a.branch3x3', 288, 384, (3, 3)), ('Mixed_6a.branch3x3dbl_1', 288, 64, (1, 1)),
          ('Mixed_6a.branch3x3dbl_2', 64, 96, (3, 3)), ('Mixed_6a.branch3x3dbl_3', 96, 96, (3, 3))]
    for n, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
        t += [(f'{n}.branch1x1', 768, 192, (1, 1)), (f'{n}.branch7x7_1', 768, c7, (1, 1)), (f'{n}.branch7x7_2', c7, c7, (1, 7)),
              (f'{n}.branch7x7_3', c7, 192, (7, 1)), (f'{n}.branch7x7dbl_1', 768, c7, (1, 1)), (f'{n}.branch7x7dbl_2', c7, c7, (7, 1)),
              (f'{n}.branch7x7dbl_3', c7, c7, (1, 7)), (f'{n}.branch7x7dbl_4', c7, c7, (7, 1)), (f'{n}.branch7x7dbl_5', c7, 192, (1, 7)),
              (f'{n}.branch_pool', 768, 192, (1, 1))]
    t += [('Mixed_7a.branch3x3_1', 768, 192, (1, 1)), ('Mixed_7a.branch3x3_2', 192, 320, (3, 3)),
          ('Mixed_7a.branch7x7x3_1', 768, 192, (1, 1)), ('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7)),
          ('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1)), ('Mixed_7a.branch7x7x3_4', 192, 192, (3, 3))]
    for n, cin in (('Mixed_7b', 1280), ('Mixed_7c', 2048)):
        t += [(f'{n}.branch1x1', cin, 320, (1, 1)), (f'{n}.branch3x3_1', cin, 384, (1, 1)), (f'{n}.branch3x3_2a', 384, 384, (1, 3)),
              (f'{n}.branch3x3_2b', 384, 384, (3, 1)), (f'{n}.branch3x3dbl_1', cin, 448, (1, 1)), (f'{n}.branch3x3dbl_2', 448, 384, (3, 3)),
              (f'{n}.branch3x3dbl_3a', 384, 384, (1, 3)), (f'{n}.branch3x3dbl_3b', 384, 384, (3, 1)), (f'{n}.branch_pool', cin, 192, (1, 1))]
    return t


TABLE = _table()


def random_state_dict(seed=0):
    """float32 CPU tensors in the torchvision key layout: He-scaled convolutions; BatchNorm statistics near the identity (gamma
    0.8..1.2, beta +-0.1, running mean +-0.05, running var 0.8..1.25), so that activations stay O(1) through all 94 layers."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, i, o, (kh, kw) in TABLE:
        sd[f'{name}.conv.weight'] = torch.randn((o, i, kh, kw), generator=g) * float(np.sqrt(2.0 / (i * kh * kw)))
        sd[f'{name}.bn.weight'] = 0.8 + 0.4 * torch.rand(o, generator=g)
        sd[f'{name}.bn.bias'] = 0.2 * torch.rand(o, generator=g) - 0.1
        sd[f'{name}.bn.running_mean'] = 0.1 * torch.rand(o, generator=g) - 0.05
        sd[f'{name}.bn.running_var'] = 0.8 + 0.45 * torch.rand(o, generator=g)
    return sd


def values_f32(images, input_range='0_255'):
    """The values the detector receives, in float32 exactly as the reference forms them: the byte / the float image ('0_255'), or
    ``real.float()*127.5 + 127.5`` ('pm1'; uint8 reals take their [-1, 1] value ``u8 / 255 * 2 - 1`` first)."""
    x = images.cpu()
    if x.dtype == torch.uint8:
        x = x.to(torch.float32)
        if input_range == 'pm1':
            x = x.div(255) * 2 - 1
    if input_range == 'pm1':
        x = x.to(torch.float32) * 127.5 + 127.5
    return x.to(torch.float32)


def resize_tf1(x, size=299):
    """TF1 legacy bilinear resize: source coordinate i * W / size, no half-pixel offset, border clamp (float64 formula)."""
    x = x.to(torch.float64)
    _, _, H, W = x.shape

    def axis(n):
        src = torch.clamp(torch.arange(size, dtype=torch.float64) * n / size, max=n - 1)
        i0 = torch.floor(src).long()
        return i0, torch.clamp(i0 + 1, max=n - 1), src - i0
    y0, y1, fy = axis(H)
    x0, x1, fx = axis(W)
    rows = x[:, :, y0, :] * (1 - fy)[:, None] + x[:, :, y1, :] * fy[:, None]
    return rows[..., x0] * (1 - fx) + rows[..., x1] * fx


def resize_grid(x, size=299):
    """The detector's form of the same resize: affine_grid with a shifted theta + grid_sample(bilinear, border, align_corners=False)."""
    B, C, H, W = x.shape
    theta = torch.eye(2, 3, dtype=x.dtype)
    theta[0, 2] += theta[0, 0] / W - theta[0, 0] / size
    theta[1, 2] += theta[1, 1] / H - theta[1, 1] / size
    theta = theta.unsqueeze(0).repeat([B, 1, 1])
    grid = F.affine_grid(theta, [B, C, size, size], align_corners=False)
    return F.grid_sample(x, grid, mode='bilinear', padding_mode='border', align_corners=False)


def frontend_f64(images, input_range='0_255'):
    x = values_f32(images, input_range).to(torch.float64)
    if tuple(x.shape[2:]) != (299, 299):
        x = resize_tf1(x)
    return (x - 128) / 128


def _cbr(sd, name, x, stride=1, pad=0):
    w = sd[f'{name}.conv.weight'].to(torch.float64)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    bn = [sd[f'{name}.bn.{k}'].to(torch.float64) for k in ('running_mean', 'running_var', 'weight', 'bias')]
    return F.relu(F.batch_norm(y, bn[0], bn[1], bn[2], bn[3], training=False, eps=EPS))


def _avg(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


def features_f64(sd, x):
    """x [B,3,299,299] float64 (after the front end) -> [B, 2048] float64."""
    c = lambda n, t, s=1, p=0: _cbr(sd, n, t, s, p)       # noqa: E731
    x = c('Conv2d_1a_3x3', x, 2)
    x = c('Conv2d_2a_3x3', x)
    x = c('Conv2d_2b_3x3', x, 1, 1)
    x = F.max_pool2d(x, 3, 2)
    x = c('Conv2d_3b_1x1', x)
    x = c('Conv2d_4a_3x3', x)
    x = F.max_pool2d(x, 3, 2)
    for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
        b1 = c(f'{n}.branch1x1', x)
        b5 = c(f'{n}.branch5x5_2', c(f'{n}.branch5x5_1', x), 1, 2)
        b3 = c(f'{n}.branch3x3dbl_3', c(f'{n}.branch3x3dbl_2', c(f'{n}.branch3x3dbl_1', x), 1, 1), 1, 1)
        bp = c(f'{n}.branch_pool', _avg(x))
        x = torch.cat([b1, b5, b3, bp], 1)
    n = 'Mixed_6a'
    b3 = c(f'{n}.branch3x3', x, 2)
    bd = c(f'{n}.branch3x3dbl_3', c(f'{n}.branch3x3dbl_2', c(f'{n}.branch3x3dbl_1', x), 1, 1), 2)
    x = torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)
    for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
        b1 = c(f'{n}.branch1x1', x)
        b7 = c(f'{n}.branch7x7_3', c(f'{n}.branch7x7_2', c(f'{n}.branch7x7_1', x), 1, (0, 3)), 1, (3, 0))
        d = c(f'{n}.branch7x7dbl_1', x)
        d = c(f'{n}.branch7x7dbl_2', d, 1, (3, 0))
        d = c(f'{n}.branch7x7dbl_3', d, 1, (0, 3))
        d = c(f'{n}.branch7x7dbl_4', d, 1, (3, 0))
        d = c(f'{n}.branch7x7dbl_5', d, 1, (0, 3))
        bp = c(f'{n}.branch_pool', _avg(x))
        x = torch.cat([b1, b7, d, bp], 1)
    n = 'Mixed_7a'
    b3 = c(f'{n}.branch3x3_2', c(f'{n}.branch3x3_1', x), 2)
    b7 = c(f'{n}.branch7x7x3_1', x)
    b7 = c(f'{n}.branch7x7x3_2', b7, 1, (0, 3))
    b7 = c(f'{n}.branch7x7x3_3', b7, 1, (3, 0))
    b7 = c(f'{n}.branch7x7x3_4', b7, 2)
    x = torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)
    for n, pool in (('Mixed_7b', _avg), ('Mixed_7c', lambda t: F.max_pool2d(t, 3, 1, 1))):
        b1 = c(f'{n}.branch1x1', x)
        a = c(f'{n}.branch3x3_1', x)
        a = torch.cat([c(f'{n}.branch3x3_2a', a, 1, (0, 1)), c(f'{n}.branch3x3_2b', a, 1, (1, 0))], 1)
        d = c(f'{n}.branch3x3dbl_2', c(f'{n}.branch3x3dbl_1', x), 1, 1)
        d = torch.cat([c(f'{n}.branch3x3dbl_3a', d, 1, (0, 1)), c(f'{n}.branch3x3dbl_3b', d, 1, (1, 0))], 1)
        bp = c(f'{n}.branch_pool', pool(x))
        x = torch.cat([b1, a, d, bp], 1)
    return x.mean(dim=(2, 3))


def detector_f64(sd, images, input_range='0_255', batch=8):
    """images [B,3,H,W] (uint8 or float32, any device) -> float64 [B, 2048] on the CPU."""
    out = []
    for b0 in range(0, images.shape[0], batch):
        out.append(features_f64(sd, frontend_f64(images[b0:b0 + batch], input_range)))
    return torch.cat(out)
