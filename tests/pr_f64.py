"""Float64 yardsticks of the improved precision / recall metric (sh-gan_amd/precision_recall.py, csrc/pr.hip) and of its VGG16 detector
(sh-gan_amd/vgg16.py, csrc/vgg16.hip).  Restatements of the documented semantics in numpy / torch float64; nothing here calls the product.

Manifold test: features rounded to fp16; distances in float64 on those rows, rounded ONCE to fp16; the (k + 1)-th smallest per row, the
point itself included; ``<=`` between fp16 values."""
import numpy as np
import torch
import torch.nn.functional as F

CONV_IDS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOL_AFTER = (1, 3, 6, 9, 12)
TORCHVISION_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
CAFFE_MEAN = (123.68, 116.779, 103.939)


def half_rows(x):
    """Any float array -> the fp16-rounded rows as float64."""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)


def dist_f64(a, b):
    """Exact-to-float64 Euclidean distances [len(a), len(b)] of fp16-representable rows (differences first: no cancellation)."""
    a, b = half_rows(a), half_rows(b)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        out[i] = np.sqrt(((a[i][None] - b) ** 2).sum(axis=1))
    return out


def dist16(a, b):
    """The distances rounded once to fp16."""
    return dist_f64(a, b).astype(np.float16)


def radii_f64(feats, k):
    """float64 radii before the fp16 rounding: the (k + 1)-th smallest distance of every row, itself included."""
    return np.sort(dist_f64(feats, feats), axis=1)[:, k]


def radii16(feats, k):
    """fp16 radii: the (k + 1)-th smallest of the fp16 distances (rounding is monotonic: the same as rounding radii_f64)."""
    return np.sort(dist16(feats, feats), axis=1)[:, k]


def inside16(probes, manifold, radii):
    return (dist16(probes, manifold) <= np.asarray(radii, dtype=np.float16)[None]).any(axis=1)


def pr16(real, fake, k):
    """-> (precision, recall)."""
    p = inside16(fake, real, radii16(real, k)).mean()
    r = inside16(real, fake, radii16(fake, k)).mean()
    return float(p), float(r)


def inside_brackets(probes, manifold, k, eps):
    """(must, may): inside with every float64 radius shrunk / grown by the relative ``eps``, distances unrounded."""
    d, r = dist_f64(probes, manifold), radii_f64(manifold, k)
    return (d <= r[None] * (1 - eps)).any(axis=1), (d <= r[None] * (1 + eps)).any(axis=1)


# ---- the detector

def random_state_dict(seed, div=8, fc=128):
    """torchvision ``vgg16`` key layout with the widths divided by ``div`` and fc layers of ``fc``; He-scaled weights so that
    activations keep their magnitude through the 15 layers, biases of both signs."""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for i, c in zip(CONV_IDS, TORCHVISION_WIDTHS):
        c //= div
        sd[f'features.{i}.weight'] = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        sd[f'features.{i}.bias'] = torch.randn(c, generator=g) * 0.1
        cin = c
    for key, (o, i) in (('classifier.0', (fc, cin * 49)), ('classifier.3', (fc, fc))):
        sd[f'{key}.weight'] = torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5
        sd[f'{key}.bias'] = torch.randn(o, generator=g) * 0.1
    return sd


def values_f64(images, input_range=None):
    """The value of every sample as the detector receives it, in float64: the byte, the float in 0..255, or (``'pm1'``) the float32
    result of ``x*127.5 + 127.5``."""
    if images.dtype == torch.uint8:
        assert input_range in (None, '0_255')
        return images.to(torch.float64)
    if input_range == 'pm1':
        return (images.to(torch.float32) * 127.5 + 127.5).to(torch.float64)
    return images.to(torch.float64)


def frontend_f64(images, input_range=None, mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0)):
    v = values_f64(images, input_range)
    if tuple(v.shape[2:]) != (224, 224):
        v = F.interpolate(v, size=(224, 224), mode='area')
    m = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return (v - m) / s


def trunk_f64(sd, x):
    for k, i in enumerate(CONV_IDS):
        x = F.relu(F.conv2d(x, sd[f'features.{i}.weight'].double(), sd[f'features.{i}.bias'].double(), padding=1))
        if k in POOL_AFTER:
            x = F.max_pool2d(x, 2)
    x = x.flatten(1)
    for key in ('classifier.0', 'classifier.3'):
        x = F.relu(F.linear(x, sd[f'{key}.weight'].double(), sd[f'{key}.bias'].double()))
    return x


def features_f64(sd, images, input_range=None, mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0)):
    return trunk_f64(sd, frontend_f64(images, input_range, mean, std))
