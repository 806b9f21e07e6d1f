"""The detector of the improved precision / recall metric: VGG16 up to ``fc2`` (the reference's lib/evaluator/stylegan_metrics/
precision_recall.py:37-46 loads it as a TorchScript download, ``vgg16.pt``, and reads ``return_features=True``), on HIP kernels.

    det = Vgg16Features.from_state_dict(torch.load('vgg16.pth'), device='cuda')          # torchvision's ``vgg16`` key layout
    feats = det(images)                                                                  # [B, F] float32, on the current stream

``images`` [B,3,H,W] of any size: uint8 (value = the byte) or float32 in 0..255; ``input_range='pm1'`` takes floats in [-1, 1] (mapped
``x*127.5 + 127.5`` in float32) or a loader's decoded uint8 pixels -- the operand rules of ``inception.InceptionFeatures``, so
``EvalLoop`` passes the same keyword.

Front end (one launch, csrc/vgg16.hip): ``F.interpolate(mode='area')`` to 224 x 224 -- adaptive average pooling over the bins
``floor(i*H/224) .. ceil((i+1)*H/224)``, exact for non-integer ratios, a copy at 224 -- then ``(v - mean_c) / std_c``.
Trunk: thirteen 3 x 3 / stride 1 / pad 1 convolutions with ReLU on the FID detector's convolution (``shg_inception_conv_f32``, exact
fp32 MFMA, ``split_k=False``), five 2 x 2 max pools (csrc/vgg16.hip), then ``relu(fc1)``, ``relu(fc2)`` on ``shg_dense_f32`` (a wave per
output feature: a weight row is read once per slab of up to 16 images, not once per image).  The output is ``relu(fc2(...))`` (a negative
pre-activation comes out as -0.0, which equals 0).  No summation order depends on the batch size: an image's features are the same
bits alone and inside any batch.

Weights: torchvision's ``vgg16`` layout -- ``features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias}``, ``classifier.{0,3}.{weight,
bias}``; ``classifier.6.*`` is ignored.  Channel and fc widths follow the tensors' shapes (a narrow net is a valid net);
``classifier.0.weight`` must be ``[F1, C5*7*7]``.

NOT verified here: the reference's ``vgg16.pt`` is a download.  The caffe-style mean (123.68, 116.779, 103.939) with unit std, the RGB
channel order and taking the features after fc2's ReLU follow the published descriptions of that detector only -- which is why ``mean``,
``std`` and ``bgr`` are constructor options.  ``bgr=True`` flips the input-channel axis of the first convolution's weights at load time (and
the mean / std with it); the image is not touched.  A torchvision ImageNet file needs ``mean = 255 * (0.485, 0.456, 0.406)``,
``std = 255 * (0.229, 0.224, 0.225)``."""
import torch

from . import _lib, inception, kernels
from ._lib import ShgError, check

RES = 224
CONV_IDS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOL_AFTER = (1, 3, 6, 9, 12)          # index into CONV_IDS of the convolution each 2 x 2 pool follows
FC_KEYS = ('classifier.0', 'classifier.3')
IGNORED_PREFIXES = ('classifier.6.',)
CAFFE_MEAN = (123.68, 116.779, 103.939)


def area_bins(size, out=RES):
    """[(start, end)] of the ``out`` bins of ``F.interpolate(mode='area')`` along an axis of ``size`` samples."""
    return [(i * size // out, -(-(i + 1) * size // out)) for i in range(out)]


def conv_walk(sd, prefixes, who):
    """The width walk over a state dict's 3 x 3 convolutions ``{prefix}.weight`` (keys present): yields (prefix, input width, output width)
    per convolution, the input width being the previous output's (3 at first).  Raises ShgError (``who``: the module in the message) at a
    weight that is no 4-D tensor with at least one output channel."""
    cin = 3
    for k in prefixes:
        w = sd[f'{k}.weight']
        if w.ndim != 4 or w.shape[0] < 1:
            raise ShgError(f"{who}: '{k}.weight' has shape {tuple(w.shape)}, expected (O, {cin}, 3, 3)")
        yield k, cin, int(w.shape[0])
        cin = int(w.shape[0])


def conv_ops(named_wb, device, bgr=False):
    """[(name, w [O,I,3,3], b [O])] float32 on the CPU, in network order (shapes validated) -> the backbone's ``inception.ConvOp`` list on
    ``device``.  ``bgr``: the net was trained on BGR planes, its input channel 0 is blue -- reading RGB images with the first weight's
    input-channel axis flipped is the same sum (the caller flips the per-channel constants, given in the net's own order, with it)."""
    ops = []
    for k, (name, w, b) in enumerate(named_wb):
        if k == 0 and bgr:
            w = w.flip(1).contiguous()
        wp, bp = inception.pack_weight(w.to(device), b.to(device))
        ops.append(inception.ConvOp(name, wp, bp, int(w.shape[1]), int(w.shape[0]), (3, 3), (1, 1), (1, 1)))
    return ops


def conv_trunk(ops, x, taps=None):
    """The backbone: x [N,3,H,W] float32, a finished network input -> the thirteen convolutions + ReLU (``split_k=False``: no launch plan
    depends on N) with a 2 x 2 max pool after those of POOL_AFTER.  ``taps=None``: the last pool's output.  ``taps``: indices into ``ops``
    -> the list of those convolutions' outputs (before the pool); a pool after the last convolution is then not run."""
    out = []
    for k, op in enumerate(ops):
        y = torch.empty((x.shape[0], op.O) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        inception.conv_group([(op, x, 0, y, 0)], split_k=False)
        if taps is not None and k in taps:
            out.append(y)
        x = maxpool2(y) if k in POOL_AFTER and (taps is None or k + 1 < len(ops)) else y
    return x if taps is None else out


def validate_state_dict(sd):
    """Raises ShgError naming the first missing key, unexpected key or wrong shape; -> (channel widths of the 13 convolutions, F1, F)."""
    keys = [f'features.{i}.{p}' for i in CONV_IDS for p in ('weight', 'bias')] + [f'{k}.{p}' for k in FC_KEYS for p in ('weight', 'bias')]
    for key in keys:
        if key not in sd:
            raise ShgError(f'vgg16: state_dict lacks {key!r}')
    for key in sd:
        if key not in keys and not key.startswith(IGNORED_PREFIXES):
            raise ShgError(f'vgg16: unexpected state_dict key {key!r}')

    def expect(key, shape):
        if tuple(sd[key].shape) != tuple(shape):
            raise ShgError(f'vgg16: {key!r} has shape {tuple(sd[key].shape)}, expected {tuple(shape)}')
    widths = []
    for key, cin, o in conv_walk(sd, [f'features.{i}' for i in CONV_IDS], 'vgg16'):
        expect(f'{key}.weight', (o, cin, 3, 3))
        expect(f'{key}.bias', (o,))
        widths.append(o)
    cin = widths[-1]
    w1, w2 = sd['classifier.0.weight'], sd['classifier.3.weight']
    if w1.ndim != 2 or w1.shape[0] < 1:
        raise ShgError(f'vgg16: \'classifier.0.weight\' has shape {tuple(w1.shape)}, expected (F1, {cin * 49})')
    expect('classifier.0.weight', (w1.shape[0], cin * 49))
    expect('classifier.0.bias', (w1.shape[0],))
    if w2.ndim != 2 or w2.shape[0] < 1:
        raise ShgError(f'vgg16: \'classifier.3.weight\' has shape {tuple(w2.shape)}, expected (F, {int(w1.shape[0])})')
    expect('classifier.3.weight', (w2.shape[0], w1.shape[0]))
    expect('classifier.3.bias', (w2.shape[0],))
    return widths, int(w1.shape[0]), int(w2.shape[0])


def frontend(images, input_range=None, mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0)):
    """images [B,3,H,W] uint8 or float32 -> [B,3,224,224] float32 = (area_resize(v) - mean_c) / std_c (one launch)."""
    input_range = '0_255' if input_range is None else input_range
    if input_range not in ('0_255', 'pm1'):
        raise ShgError(f"vgg16: input_range must be None, '0_255' or 'pm1' (got {input_range!r})")
    L = kernels._Launch()
    x, lut, scale, bias = kernels._image_operand(L, images, 'images', lambda dev: inception.value_table(dev, input_range),
                                                 (127.5, 127.5) if input_range == 'pm1' else (1.0, 0.0), 'vgg16')
    B, _, H, W = x.shape
    y = L.new((B, 3, RES, RES))
    with L:
        check(_lib.get_lib().shg_vgg16_frontend_f32(kernels._ptr(x), kernels._ptr(lut), scale, bias, kernels._c3(mean), kernels._c3(std),
                                                    kernels._ptr(y), B, H, W, L.stream()), 'vgg16_frontend')
    return y


def maxpool2(x):
    """2 x 2 max pool, stride 2 (floor) of a float32 [B,C,H,W] tensor (one launch)."""
    L = kernels._Launch()
    x = L.req(x, 'x')
    if x.ndim != 4:
        raise ShgError(f'vgg16: maxpool2 takes [B,C,H,W] (got {tuple(x.shape)})')
    B, C, H, W = x.shape
    y = L.new((B, C, H // 2, W // 2))
    with L:
        check(_lib.get_lib().shg_vgg16_maxpool2_f32(kernels._ptr(x), kernels._ptr(y), B, C, H, W, L.stream()), 'vgg16_maxpool2')
    return y


def fc_relu(x, w, b):
    """relu(x [B,K] @ w [O,K].T + b [O]) on shg_dense_f32 (leaky-ReLU of slope 0)."""
    L = kernels._Launch()
    x, w, b = L.req(x, 'x'), L.req(w, 'w'), L.req(b, 'bias')
    if x.ndim != 2 or w.ndim != 2 or x.shape[1] != w.shape[1] or tuple(b.shape) != (w.shape[0],):
        raise ShgError(f'vgg16: fc operands {tuple(x.shape)}, {tuple(w.shape)}, {tuple(b.shape)} do not fit')
    N, K, O = x.shape[0], x.shape[1], w.shape[0]
    y = L.new((N, O))
    with L:
        check(_lib.get_lib().shg_dense_f32(kernels._ptr(x), kernels._ptr(w), kernels._ptr(b), kernels._ptr(y), N, K, O, K, O, 1.0, 1.0, 1, 0.0, 1.0,
                                           -1.0, L.stream()), 'vgg16_fc')
    return y


def macs_per_image(widths, f1, f):
    """Multiply-adds of the 13 convolutions and the two fc layers for one 224 x 224 image."""
    total, cin, side = 0, 3, RES
    for k, c in enumerate(widths):
        total += side * side * c * cin * 9
        cin = c
        if k in POOL_AFTER:
            side //= 2
    return total + cin * 49 * f1 + f1 * f


class Vgg16Features:
    """``det(images, input_range=None) -> [B, F]`` float32, F = the width of fc2.  Every launch goes to the current stream and every
    buffer comes from torch's caching allocator on it (EvalLoop's side streams)."""

    def __init__(self, ops, fcs, widths, mean, std, device):
        self.ops, self.fcs, self.widths = ops, fcs, tuple(widths)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.device = torch.device(device)
        self.dim = int(fcs[1][0].shape[0])

    @classmethod
    def from_state_dict(cls, sd, device='cuda', mean=CAFFE_MEAN, std=(1.0, 1.0, 1.0), bgr=False):
        widths, _, _ = validate_state_dict(sd)
        if len(mean) != 3 or len(std) != 3 or min(float(s) for s in std) <= 0:
            raise ShgError(f'vgg16: mean and std must be three numbers each, std positive (got {mean!r}, {std!r})')
        dev = torch.device(device)
        f32 = lambda t: torch.as_tensor(t).detach().cpu().to(torch.float32).contiguous()      # noqa: E731
        ops = conv_ops([(f'features.{i}', f32(sd[f'features.{i}.weight']), f32(sd[f'features.{i}.bias'])) for i in CONV_IDS], dev, bgr)
        fcs = [(f32(sd[f'{k}.weight']).to(dev), f32(sd[f'{k}.bias']).to(dev)) for k in FC_KEYS]
        if bgr:
            mean, std = tuple(mean)[::-1], tuple(std)[::-1]
        return cls(ops, fcs, widths, mean, std, dev)

    def trunk(self, x):
        """x [B,3,224,224] normalised -> [B, F]."""
        x = conv_trunk(self.ops, x).reshape(x.shape[0], -1)
        for w, b in self.fcs:
            x = fc_relu(x, w, b)
        return x

    def __call__(self, images, input_range=None):
        if not isinstance(images, torch.Tensor) or not images.is_cuda:
            raise ShgError('vgg16: images must reside on a HIP (cuda) device: there is no CPU path')
        with torch.no_grad():
            return self.trunk(frontend(images, input_range, self.mean, self.std))
