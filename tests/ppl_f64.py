"""Test helper: the yardstick of tests/test_ppl_cpu.py and tests/test_gpu_ppl.py -- CPU restatements of everything sh-gan_amd/ppl.py and
``lpips.LPIPS(net='vgg')`` compute, written from the reference's lib/evaluator/stylegan_metrics/perceptual_path_length.py and the published
LPIPS / VGG16 architecture in plain numpy / ``torch.nn.functional`` calls.  Nothing here is shipped and nothing here is a test.

Every network restatement takes a ``dtype``: float64 is the yardstick; the SAME code in float32 on the CPU measures the reference
arithmetic's own distance from it (``dist`` is a difference of nearly equal feature vectors: its float32 error is set by cancellation,
not by which float32 implementation ran).  The plain StyleGAN2 synthesis is composed from the layer functions of oracle/shgan_oracle.py
(which follow their operands' dtype)."""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_f64
from oracle import shgan_oracle as orc

CAFFE_MEAN = (123.68, 116.779, 103.939)
VGG_CONV_IDS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_SLICE_OF = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
VGG_TAPS = (1, 3, 6, 9, 12)
NARROW = (8, 8, 16, 16, 24, 24, 24, 32, 32, 32, 32, 32, 32)


# ---- front end (perceptual_path_length.py:71-85 + the detector's normalisation) ----------------------------------------------------------------

def window(x, crop):
    """:72-75 on a numpy / torch [N,C,R,R] array."""
    if not crop:
        return x
    c = x.shape[2] // 8
    return x[:, :, c * 3:c * 7, c * 2:c * 6]


def box_mean_f64(x, factor, crop):
    """float32 x [N,C,R,R] -> float64 [N,C,S,S]: the exact box means (:78-80) of the float32 values."""
    v = np.asarray(window(x, crop), dtype=np.float64)
    f = max(int(factor), 1)
    n, c, h, w = v.shape
    return v.reshape(n, c, h // f, f, w // f, f).mean(axis=(3, 5)) if f > 1 else v


def frontend_steps_f32(m32, mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0)):
    """float32 means [N,C,S,S] -> float32 [N,3,S,S]: the reference's float32 steps (m + 1) * (255 / 2) (:83), the grey repeat (:84-85) and
    the detector's (u - mean_c) / std_c, every operation rounded to float32 once."""
    m32 = np.asarray(m32, dtype=np.float32)
    u = (m32 + np.float32(1)) * np.float32(255 / 2)
    if u.shape[1] == 1:
        u = np.repeat(u, 3, axis=1)
    mean = np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1)
    std = np.asarray(std, dtype=np.float32).reshape(1, 3, 1, 1)
    return ((u - mean) / std).astype(np.float32)


def frontend_candidates(x, factor, crop, mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0)):
    """-> (below, exact, above) float32 [N,3,S,S]: the float32 steps applied to the float64 box mean rounded to float32 and to its two
    float32 neighbours -- "the mean may differ in the last place", everything after it is determined."""
    m = box_mean_f64(x, factor, crop).astype(np.float32)
    lo, hi = np.nextafter(m, np.float32(-np.inf)), np.nextafter(m, np.float32(np.inf))
    return tuple(frontend_steps_f32(v, mean, std) for v in (lo, m, hi))


def frontend_t(img, factor, crop, mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0)):
    """The same front end on a torch tensor in ITS dtype (float64: the yardstick; float32: the reference's four passes)."""
    img = window(img, crop)
    f = max(int(factor), 1)
    if f > 1:
        img = img.reshape([-1, img.shape[1], img.shape[2] // f, f, img.shape[3] // f, f]).mean([3, 5])
    img = (img + 1) * (255 / 2)
    if img.shape[1] == 1:
        img = img.repeat([1, 3, 1, 1])
    mean = torch.tensor(mean, dtype=torch.float32).to(img.dtype).reshape(1, 3, 1, 1)
    std = torch.tensor(std, dtype=torch.float32).to(img.dtype).reshape(1, 3, 1, 1)
    return (img - mean) / std


# ---- LPIPS with the VGG16 backbone ---------------------------------------------------------------------------------------------------------------

def vgg_random_state_dict(widths=NARROW, seed=0, layout='package'):
    """float32 CPU tensors: He-scaled 3 x 3 convolutions, biases 0.1 * randn, ``lin`` weights rand * 2 / C.  layout 'package': the
    ``lpips`` package's keys in one dict; 'features': (torchvision ``vgg16`` dict, ``vgg.pth`` lin dict)."""
    g = torch.Generator().manual_seed(int(seed))
    conv, lin, cin = {}, {}, 3
    for s, i, c in zip(VGG_SLICE_OF, VGG_CONV_IDS, widths):
        key = f'net.slice{s}.{i}' if layout == 'package' else f'features.{i}'
        conv[f'{key}.weight'] = torch.randn((c, cin, 3, 3), generator=g) * float(np.sqrt(2.0 / (cin * 9)))
        conv[f'{key}.bias'] = 0.1 * torch.randn(c, generator=g)
        cin = c
    for n, t in enumerate(VGG_TAPS):
        lin[f'lin{n}.model.1.weight'] = torch.rand((1, widths[t], 1, 1), generator=g) * 2 / widths[t]
    if layout == 'package':
        conv.update(lin)
        return conv
    return conv, lin


def vgg_taps(sd, x, dtype=torch.float64):
    """A finished network input [N,3,H,W] -> the five taps (relu1_2, 2_2, 3_3, 4_3, 5_3) in ``dtype``."""
    x, taps = x.to(dtype), []
    for k, (s, i) in enumerate(zip(VGG_SLICE_OF, VGG_CONV_IDS)):
        key = f'net.slice{s}.{i}'
        x = F.relu(F.conv2d(x, sd[f'{key}.weight'].to(dtype), sd[f'{key}.bias'].to(dtype), padding=1))
        if k in VGG_TAPS:
            taps.append(x)
            if k != VGG_TAPS[-1]:
                x = F.max_pool2d(x, 2, 2)
    return taps


def head(fp, fg, w):
    """One tap in the operands' dtype -> [B]: the spatial mean of sum_c w_c (f^_p - f^_g)^2."""
    w = w.to(fp.dtype).reshape(1, -1, 1, 1)
    n0 = fp / (torch.sqrt((fp ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    n1 = fg / (torch.sqrt((fg ** 2).sum(dim=1, keepdim=True)) + 1e-10)
    return (w * (n0 - n1) ** 2).sum(dim=1).mean(dim=(1, 2))


def distance(sd, x, dtype=torch.float64):
    """x [2B,3,H,W] finished inputs -> [B]: image b against image B + b, summed over the five taps."""
    B = x.shape[0] // 2
    return sum(head(t[:B], t[B:], sd[f'lin{n}.model.1.weight']) for n, t in enumerate(vgg_taps(sd, x, dtype)))


def lpips_vgg(sd, pred, gt, gt_range='pm1', dtype=torch.float64):
    """pred / gt in the forms ``Lpips.__call__`` takes -> [B] on the CPU: the float32 operand values of the evaluator batch
    (tests/lpips_f64.py), then the scaling layer, trunk and heads in ``dtype``."""
    v = torch.cat([lpips_f64.pred_values_f32(pred), lpips_f64.gt_values_f32(gt, gt_range)])
    sh = torch.tensor(lpips_f64.SHIFT, dtype=torch.float32).to(dtype)[None, :, None, None]
    sc = torch.tensor(lpips_f64.SCALE, dtype=torch.float32).to(dtype)[None, :, None, None]
    return distance(sd, (v.to(dtype) - sh) / sc, dtype)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------------

def slerp(a, b, t):
    """:22-31."""
    a = a / a.norm(dim=-1, keepdim=True)
    b = b / b.norm(dim=-1, keepdim=True)
    d = (a * b).sum(dim=-1, keepdim=True)
    p = t * torch.acos(d)
    c = b - d * a
    c = c / c.norm(dim=-1, keepdim=True)
    d = a * torch.cos(p) + c * torch.sin(p)
    return d / d.norm(dim=-1, keepdim=True)


def mapping(sd, z, num_ws, num_layers, lr_multi=0.01):
    """model_zoo/stylegan.py ``Mapping`` (c_dim 0, truncation 1, eval) in z's dtype."""
    x = z * (z.square().mean(dim=1, keepdim=True) + 1e-8).rsqrt()
    for i in range(num_layers):
        x = orc.dense(x, sd[f'mapping.fc{i}.weight'], sd[f'mapping.fc{i}.bias'], lr_multi=lr_multi, act=True)
    return x.unsqueeze(1).repeat(1, num_ws, 1)


def synthesis(sd, ws, resolution, noise):
    """The plain ``Synthesis`` (const input, skip architecture, noise_mode='const' with the given ``noise`` {layer prefix: [r, r]}) in the
    dtype of ``sd`` / ``ws``."""
    sd = dict(sd)
    for p, v in noise.items():
        sd[p + 'noise_const'] = v
    x = img = None
    k = 0
    for res in [2 ** i for i in range(2, int(np.log2(resolution)) + 1)]:
        p = f'synthesis.b{res}.'
        if res == 4:
            x = sd[p + 'const'].unsqueeze(0).repeat(ws.shape[0], 1, 1, 1)
        else:
            x = orc.synthesis_layer(sd, p + 'conv0.', x, ws[:, k], res, up=2)
            k += 1
        x = orc.synthesis_layer(sd, p + 'conv1.', x, ws[:, k], res)
        k += 1
        y = orc.torgb_layer(sd, p + 'torgb.', x, ws[:, k])
        img = y if img is None else orc.upsample2d(img, sd[p + 'resample_filter']) + y
    return img


def sampler_dist(G_sd, vgg_sd, draws, resolution, num_layers, epsilon=1e-4, space='w', crop=False, mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0),
                 dtype=torch.float64):
    """The whole of ``PPLSampler.forward`` (:48-90) from given draws {'t': [B], 'z0', 'z1': [B, z_dim], 'noise': {prefix: [r, r]}} (float32, as
    the device drew them) -> dist [B], everything after the draws in ``dtype``."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in G_sd.items()}
    t, z0, z1 = (draws[k].to(dtype) for k in ('t', 'z0', 'z1'))
    num_ws = 2 * int(np.log2(resolution)) - 2
    if space == 'w':
        w0, w1 = mapping(sd, torch.cat([z0, z1]), num_ws, num_layers).chunk(2)
        tt = t.unsqueeze(1).unsqueeze(2)
        wt0, wt1 = w0.lerp(w1, tt), w0.lerp(w1, tt + epsilon)
    else:
        zt0, zt1 = slerp(z0, z1, t.unsqueeze(1)), slerp(z0, z1, t.unsqueeze(1) + epsilon)
        wt0, wt1 = mapping(sd, torch.cat([zt0, zt1]), num_ws, num_layers).chunk(2)
    img = synthesis(sd, torch.cat([wt0, wt1]), resolution, {p: v.to(dtype) for p, v in draws['noise'].items()})
    x = frontend_t(img, resolution // 256, crop, mean, std)
    return distance(vgg_sd, x, dtype) / epsilon ** 2


# ---- the metric's tail -----------------------------------------------------------------------------------------------------------------------------

def trimmed_mean_np(dist):
    """:124-127 with numpy's current spelling of ``interpolation=``."""
    dist = np.asarray(dist, dtype=np.float64)
    lo = np.percentile(dist, 1, method='lower')
    hi = np.percentile(dist, 99, method='higher')
    return float(np.extract(np.logical_and(dist >= lo, dist <= hi), dist).mean())


def interleave_np(per_rank, batch_size, num_samples):
    """per_rank: the ranks' lists of per-call [B] arrays -> the reference's ``torch.cat(dist)[:num_samples]`` (:113-118, :124)."""
    out = []
    for r in range(len(per_rank[0])):
        for src in range(len(per_rank)):
            out.append(np.asarray(per_rank[src][r]))
    return np.concatenate(out)[:num_samples]
