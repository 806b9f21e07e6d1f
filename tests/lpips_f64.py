"""Test helper: a float64 CPU model of ``lpips.LPIPS(net='alex')`` (version 0.1, spatial=False) as the reference's eva_lpips.py:39-52
calls it, written from the published architecture in plain ``torch.nn.functional`` calls, and random weights from a seed in the package's
key layout.  The model takes the FLOAT32 operand values the evaluator batch holds (shgan_default.py:283-286, eva_lpips.py:39-45) and does
everything after them in float64.  Nothing here is shipped; it is the yardstick of tests/test_*lpips*.py.  The reference's own evaluator
cannot produce a fixture (``import lpips`` fails where this was written), so there is no golden file."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (package key, I, O, kernel, stride, pad)
CONVS = (('net.slice1.0', 3, 64, 11, 4, 2), ('net.slice2.3', 64, 192, 5, 1, 2), ('net.slice3.6', 192, 384, 3, 1, 1),
         ('net.slice4.8', 384, 256, 3, 1, 1), ('net.slice5.10', 256, 256, 3, 1, 1))


def random_state_dict(seed=0):
    """float32 CPU tensors in the package's key layout: He-scaled convolutions, biases 0.1 * randn, ``lin`` weights rand * 2 / C
    (non-negative, as the trained ones are)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for key, i, o, k, _, _ in CONVS:
        sd[f'{key}.weight'] = torch.randn((o, i, k, k), generator=g) * float(np.sqrt(2.0 / (i * k * k)))
        sd[f'{key}.bias'] = 0.1 * torch.randn(o, generator=g)
    for n, (_, _, o, _, _, _) in enumerate(CONVS):
        sd[f'lin{n}.model.1.weight'] = torch.rand((1, o, 1, 1), generator=g) * 2 / o
    return sd


def pred_values_f32(pred):
    """The network's ``pred`` operand: uint8 composite -> float32(((u8 / 255) - 0.5) * 2) with numpy float64 inside; float32 in [0, 1] ->
    (x - 0.5) * 2 in float32."""
    pred = pred.cpu()
    if pred.dtype == torch.uint8:
        return torch.from_numpy((((pred.numpy() / 255) - 0.5) * 2).astype(np.float32))
    return (pred.to(torch.float32) - 0.5) * 2


def gt_values_f32(gt, gt_range='pm1'):
    """The network's ``gt`` operand, float32 throughout: 'pm1' real in [-1, 1] (uint8 pixels: ToTensor / 255 then * 2 - 1) ->
    ((real + 1) / 2 - 0.5) * 2; 'unit': values in [0, 1] (uint8: float32(u8 / 255)) -> (u - 0.5) * 2."""
    gt = gt.cpu()
    if gt_range == 'pm1':
        real = gt.to(torch.float32).div(255) * 2 - 1 if gt.dtype == torch.uint8 else gt.to(torch.float32)
        u = (real + 1) / 2
    else:
        u = torch.from_numpy((gt.numpy() / 255).astype(np.float32)) if gt.dtype == torch.uint8 else gt.to(torch.float32)
    return (u - 0.5) * 2


def scaling_f64(v, shift=SHIFT, scale=SCALE):
    """float32 operand values -> float64 (v - shift) / scale with the float32 constants of the scaling layer's buffers."""
    sh = torch.tensor(shift, dtype=torch.float32).to(torch.float64)[None, :, None, None]
    sc = torch.tensor(scale, dtype=torch.float32).to(torch.float64)[None, :, None, None]
    return (v.to(torch.float64) - sh) / sc


def conv1_f64(sd, v):
    key = CONVS[0][0]
    return F.relu(F.conv2d(scaling_f64(v), sd[f'{key}.weight'].to(torch.float64), sd[f'{key}.bias'].to(torch.float64), stride=4, padding=2))


def taps_f64(sd, v):
    """float32 operand values [B,3,H,W] -> the five taps (float64)."""
    taps = []
    x = scaling_f64(v)
    for n, (key, _, _, _, s, p) in enumerate(CONVS):
        if n in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[f'{key}.weight'].to(torch.float64), sd[f'{key}.bias'].to(torch.float64), stride=s, padding=p))
        taps.append(x)
    return taps


def head_f64(fp, fg, w):
    """One tap: features [B,C,h,w], w [C] -> float64 [B], the spatial mean of sum_c w_c (f^_pred - f^_gt)^2."""
    fp, fg, w = fp.to(torch.float64), fg.to(torch.float64), w.to(torch.float64).reshape(1, -1, 1, 1)
    n0 = fp / (torch.sqrt((fp ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    n1 = fg / (torch.sqrt((fg ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    return (w * (n0 - n1) ** 2).sum(dim=1).mean(dim=(1, 2))


def lpips_f64(sd, pred, gt, gt_range='pm1', batch=4):
    """pred / gt in the forms ``Lpips.__call__`` takes (any device) -> float64 [B] on the CPU."""
    out = []
    for b0 in range(0, pred.shape[0], batch):
        tp = taps_f64(sd, pred_values_f32(pred[b0:b0 + batch]))
        tg = taps_f64(sd, gt_values_f32(gt[b0:b0 + batch], gt_range))
        out.append(sum(head_f64(a, b, sd[f'lin{n}.model.1.weight']) for n, (a, b) in enumerate(zip(tp, tg))))
    return torch.cat(out)


def image_pairs(B, H, W, seed, holes=(0.02, 0.30, 0.50)):
    """The composite's form: ``real`` = a bilinearly upsampled random field plus noise, ``pred`` = ``real`` with a square hole (a fraction
    of the area, cycling through ``holes``) filled with other noise.  -> (pred_u8, real_u8) uint8 [B,3,H,W]."""
    g = torch.Generator().manual_seed(int(seed))
    field = torch.rand(B, 3, max(2, H // 16), max(2, W // 16), generator=g)
    real = F.interpolate(field, size=(H, W), mode='bilinear', align_corners=False) * 0.8 + 0.1 + 0.05 * torch.randn(B, 3, H, W, generator=g)
    real_u8 = (real.clamp(0, 1) * 255).round().to(torch.uint8)
    pred_u8 = real_u8.clone()
    for b in range(B):
        frac = holes[(b + seed) % len(holes)]
        hh, hw = max(1, int(round(H * frac ** 0.5))), max(1, int(round(W * frac ** 0.5)))
        y0, x0 = (H - hh) // 3, (W - hw) // 2
        pred_u8[b, :, y0:y0 + hh, x0:x0 + hw] = torch.randint(0, 256, (3, hh, hw), generator=g, dtype=torch.uint8)
    return pred_u8, real_u8
