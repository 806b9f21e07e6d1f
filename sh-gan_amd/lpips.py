"""LPIPS with the AlexNet backbone -- ``lpips.LPIPS(net='alex')`` (version 0.1, ``spatial=False``, ``lpips=True``) as the reference's
lib/evaluator/eva_lpips.py:39-52 calls it -- on the HIP kernels of csrc/lpips.hip (first convolution, distance head) and
csrc/inception.hip (conv2..conv5, the max pools).

    net = Lpips.from_state_dict(torch.load('lpips_alex_full.pth'), device='cuda')     # or from_state_dicts(alexnet_sd, lin_sd)
    v = net(pred_u8, real)                                                              # float64 [B], on the current stream

The ``lpips`` package cannot be imported where this was written; what follows restates its PUBLISHED source and was not run against it:

1. operands ``pred``, ``gt`` in [-1, 1], float32, at the images' own size (no resize);
2. scaling layer ``(x - shift) / scale``, shift (-.030, -.088, -.188), scale (.458, .448, .450) per channel;
3. AlexNet ``features``: conv 3->64 k11 s4 p2 + ReLU (tap 0), maxpool 3 s2, conv 64->192 k5 p2 + ReLU (tap 1), maxpool 3 s2, conv
   192->384 k3 p1 + ReLU (tap 2), conv 384->256 k3 p1 + ReLU (tap 3), conv 256->256 k3 p1 + ReLU (tap 4); all with bias, floor pools;
4. per tap and pixel ``f^ = f / (sqrt(sum_c f^2) + 1e-10)`` for both images and ``d = sum_c w_c (f^_pred - f^_gt)^2`` with the tap's
   ``lin`` weight (a 1 x 1 convolution to one channel without bias; the dropout in front of it is off in eval);
5. value = sum over the five taps of the spatial mean of ``d``: one number per image pair.

Operand values follow the evaluator batch (shgan_default.py:283-286, eva_lpips.py:39-45): ``pred = float32(((u8 / 255) - 0.5) * 2)`` with
the inner arithmetic in float64 (numpy), ``gt = ((real + 1) / 2 - 0.5) * 2`` in float32 throughout.  uint8 operands take these from
256-entry tables, float32 operands from the same float32 steps inside the kernel's load.  The one departure from the published arithmetic:
the scaling layer multiplies by ``float32(1 / scale)`` instead of dividing (at most one ulp of the operand).

Weights (``from_state_dict``): the package's own layout -- ``net.slice1.0.{weight,bias}``, ``net.slice2.3.*``, ``net.slice3.6.*``,
``net.slice4.8.*``, ``net.slice5.10.*``, ``lin{0..4}.model.1.weight`` [1,C,1,1], optionally the duplicates ``lins.{k}.model.1.weight`` and
``scaling_layer.{shift,scale}`` (else the constants above) -- or (``from_state_dicts``) torchvision's ``alexnet`` state_dict
(``features.{0,3,6,8,10}.{weight,bias}``; ``classifier.*`` ignored) plus the package's ``alex.pth`` (``lin{k}.model.1.weight``).  Both
layouts were written from the published sources and NOT checked against the files, which are downloads and are not shipped.

Pred and gt go through the network as one batch of 2B.  No launch plan depends on the batch size (``split_k=False``), the head adds in a
fixed order without atomics: a pair's value is the same bits alone and inside any batch.

``net='vgg'`` (``LPIPS(net='vgg', ...)``, ``Lpips.from_state_dict(sd, net='vgg')``): the same class, operands, call and guarantees with the
VGG16 backbone -- the thirteen 3 x 3 convolutions and 2 x 2 max pools of vgg16.py, taps after the ReLU of convolutions 1, 3, 6, 9 and 12
of ``vgg16.CONV_IDS`` (relu1_2, 2_2, 3_3, 4_3, 5_3) before the pool that follows each, five ``lin`` vectors of the taps' widths.  The
scaling layer is a pass of its own there (``scaling``: csrc/lpips.hip, the float32 steps of conv1's load), the convolutions run on
``inception.conv_group(..., split_k=False)``, the pools on ``vgg16.maxpool2``; channel widths follow the tensors (a narrow net is a valid
net); images of at least 16 x 16.  Keys: the package's ``net.slice1.{0,2}``, ``net.slice2.{5,7}``, ``net.slice3.{10,12,14}``,
``net.slice4.{17,19,21}``, ``net.slice5.{24,26,28}`` ``.{weight,bias}`` + ``lin{0..4}.model.1.weight``, or torchvision's ``vgg16``
``features.*`` (``classifier.*`` ignored) plus the package's ``vgg.pth``.  Like the alex layouts they were written from the published
sources and NOT checked against the files.  ``mean`` / ``std`` / ``bgr`` are the constants of ``trunk``'s other caller, the path-length
sampler (ppl.py), whose detector takes 0..255 images normalised as ``vgg16.Vgg16Features`` does; ``bgr=True`` flips the input-channel
axis of the first convolution at load time and every per-channel constant (mean, std, shift, scale: given in the net's own order) with it."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, inception, kernels, vgg16
from ._lib import ShgError, check

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (I, O, kernel, stride, pad) of AlexNet's five convolutions; every one is a tap
CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
TAP_CHANNELS = tuple(c[1] for c in CONVS)
PACKAGE_CONV_KEYS = ('net.slice1.0', 'net.slice2.3', 'net.slice3.6', 'net.slice4.8', 'net.slice5.10')
ALEXNET_CONV_KEYS = ('features.0', 'features.3', 'features.6', 'features.8', 'features.10')
MIN_SIZE = 31             # the second max pool must see 3 x 3
NETS = ('alex', 'vgg')
VGG_TAPS = vgg16.POOL_AFTER               # index into vgg16.CONV_IDS of the convolution each tap follows (the one before every pool)
VGG_SLICE_OF = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
VGG_PACKAGE_CONV_KEYS = tuple(f'net.slice{s}.{i}' for s, i in zip(VGG_SLICE_OF, vgg16.CONV_IDS))
VGG_FEATURES_CONV_KEYS = tuple(f'features.{i}' for i in vgg16.CONV_IDS)
VGG_MIN_SIZE = 16         # four pools before the last tap


def out_sizes(h):
    """Side of the five taps for an input side h."""
    t0 = inception.out_size(h, 11, 4, 2)
    t1 = inception.out_size(t0, 3, 2, 0)
    t2 = inception.out_size(t1, 3, 2, 0)
    return (t0, t1, t2, t2, t2)


def macs_per_pair(H, W):
    """Multiply-adds of the ten convolutions of one (pred, gt) pair at H x W (pools and the head are not counted)."""
    hs, ws = out_sizes(H), out_sizes(W)
    return 2 * sum(hs[k] * ws[k] * o * i * ks * ks for k, (i, o, ks, _, _) in enumerate(CONVS))


def _conv_shapes(prefixes):
    want = collections.OrderedDict()
    for key, (i, o, k, _, _) in zip(prefixes, CONVS):
        want[f'{key}.weight'] = (o, i, k, k)
        want[f'{key}.bias'] = (o,)
    return want


def _lin_shapes():
    return collections.OrderedDict((f'lin{k}.model.1.weight', (1, c, 1, 1)) for k, c in enumerate(TAP_CHANNELS))


def _validate(sd, want, optional, ignored_prefixes, what):
    for key in want:
        if key not in sd:
            raise ShgError(f'lpips: {what} lacks {key!r}')
    for key, t in sd.items():
        if key.startswith(ignored_prefixes):
            continue
        shape = want.get(key, optional.get(key))
        if shape is None:
            raise ShgError(f'lpips: unexpected {what} key {key!r}')
        if tuple(t.shape) != shape:
            raise ShgError(f'lpips: {key!r} has shape {tuple(t.shape)}, expected {shape}')


def validate_state_dict(sd):
    """The package's layout.  Raises ShgError naming the first missing key, unexpected key or wrong shape."""
    want = _conv_shapes(PACKAGE_CONV_KEYS)
    want.update(_lin_shapes())
    optional = {f'lins.{k}.model.1.weight': (1, c, 1, 1) for k, c in enumerate(TAP_CHANNELS)}
    optional.update({'scaling_layer.shift': (1, 3, 1, 1), 'scaling_layer.scale': (1, 3, 1, 1)})
    _validate(sd, want, optional, (), 'state_dict')


def validate_state_dicts(alexnet_sd, lin_sd):
    """The two-file layout: torchvision ``alexnet`` (``classifier.*`` ignored) and the package's ``alex.pth``."""
    _validate(alexnet_sd, _conv_shapes(ALEXNET_CONV_KEYS), {}, ('classifier.',), 'alexnet state_dict')
    _validate(lin_sd, _lin_shapes(), {}, (), 'lin state_dict')


def _f32(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float32).contiguous()


def _canonical(sd, lin_sd, prefixes, out, lin_after_conv):
    """The tail both backbones share: the convolutions under ``prefixes``, the five ``lin`` vectors (the one-file layout's ``lins.*``
    duplicates must agree) and the scaling layer's constants (the one-file layout may carry its own) -> ``out``.  Key order:
    ``lin{k}`` behind ``conv{k}`` (alex: a tap per convolution) or the five behind all convolutions (vgg), as each layout always had it."""
    full = lin_sd is None
    lins = sd if full else lin_sd

    def lin(n):
        out[f'lin{n}'] = _f32(lins[f'lin{n}.model.1.weight']).reshape(-1)
        dup = f'lins.{n}.model.1.weight'
        if full and dup in sd and not torch.equal(_f32(sd[dup]).reshape(-1), out[f'lin{n}']):
            raise ShgError(f'lpips: {dup!r} differs from its duplicate \'lin{n}.model.1.weight\'')
    for k, key in enumerate(prefixes):
        out[f'conv{k}.weight'] = _f32(sd[f'{key}.weight'])
        out[f'conv{k}.bias'] = _f32(sd[f'{key}.bias'])
        if lin_after_conv:
            lin(k)
    if not lin_after_conv:
        for n in range(5):
            lin(n)
    out['shift'] = _f32(sd['scaling_layer.shift']).reshape(-1) if full and 'scaling_layer.shift' in sd else torch.tensor(SHIFT)
    out['scale'] = _f32(sd['scaling_layer.scale']).reshape(-1) if full and 'scaling_layer.scale' in sd else torch.tensor(SCALE)
    return out


def canonical_weights(sd, lin_sd=None):
    """Either layout (validated) -> {'conv{k}.weight', 'conv{k}.bias', 'lin{k}' [C], 'shift' [3], 'scale' [3]} float32 on the CPU."""
    if lin_sd is None:
        validate_state_dict(sd)
    else:
        validate_state_dicts(sd, lin_sd)
    return _canonical(sd, lin_sd, PACKAGE_CONV_KEYS if lin_sd is None else ALEXNET_CONV_KEYS, collections.OrderedDict(), True)


def _validate_vgg(sd, lins, prefixes, ignored_prefixes, what, lin_what):
    """Widths follow the tensors: -> the 13 channel widths.  Raises ShgError naming the first missing key, unexpected key or wrong shape."""
    conv_keys = [f'{k}.{p}' for k in prefixes for p in ('weight', 'bias')]
    lin_keys = [f'lin{k}.model.1.weight' for k in range(5)]
    same = lins is sd
    for key in conv_keys + (lin_keys if same else []):
        if key not in sd:
            raise ShgError(f'lpips: {what} lacks {key!r}')
    widths, shapes = [], {}
    for k, cin, o in vgg16.conv_walk(sd, prefixes, 'lpips'):
        shapes[f'{k}.weight'], shapes[f'{k}.bias'] = (o, cin, 3, 3), (o,)
        widths.append(o)
    lin_shapes = {f'lin{n}.model.1.weight': (1, widths[t], 1, 1) for n, t in enumerate(VGG_TAPS)}
    optional = {}
    if same:
        shapes.update(lin_shapes)
        optional = {f'lins.{n}.model.1.weight': (1, widths[t], 1, 1) for n, t in enumerate(VGG_TAPS)}
        optional.update({'scaling_layer.shift': (1, 3, 1, 1), 'scaling_layer.scale': (1, 3, 1, 1)})
    _validate(sd, shapes, optional, ignored_prefixes, what)
    if not same:
        _validate(lins, lin_shapes, {}, (), lin_what)
    return widths


def validate_vgg_state_dict(sd):
    """The package's ``LPIPS(net='vgg')`` layout -> the 13 channel widths."""
    return _validate_vgg(sd, sd, VGG_PACKAGE_CONV_KEYS, (), 'state_dict', None)


def validate_vgg_state_dicts(vgg_sd, lin_sd):
    """The two-file layout: torchvision ``vgg16`` (``classifier.*`` ignored) and the package's ``vgg.pth`` -> the 13 channel widths."""
    return _validate_vgg(vgg_sd, lin_sd, VGG_FEATURES_CONV_KEYS, ('classifier.',), 'vgg16 state_dict', 'lin state_dict')


def canonical_vgg_weights(sd, lin_sd=None):
    """Either vgg layout (validated) -> {'conv{k}.weight', 'conv{k}.bias' (k < 13), 'lin{n}' [C_n], 'shift', 'scale', 'widths'} on the CPU."""
    if lin_sd is None:
        widths, prefixes = validate_vgg_state_dict(sd), VGG_PACKAGE_CONV_KEYS
    else:
        widths, prefixes = validate_vgg_state_dicts(sd, lin_sd), VGG_FEATURES_CONV_KEYS
    return _canonical(sd, lin_sd, prefixes, collections.OrderedDict(widths=tuple(widths)), False)


def vgg_out_sizes(h):
    """Side of the five vgg taps for an input side h (2 x 2 floor pools)."""
    return tuple(h >> k for k in range(5))


def vgg_macs_per_image(widths, H, W):
    """Multiply-adds of the thirteen convolutions of ONE image at H x W."""
    total, cin, h, w = 0, 3, H, W
    for k, c in enumerate(widths):
        total += h * w * c * cin * 9
        cin = c
        if k in VGG_TAPS:
            h, w = h // 2, w // 2
    return total


def value_table_cpu(operand, gt_range='pm1'):
    """float32 [256]: the value of every uint8 code as the network receives it.  'pred': the composite, ``float32(((u8 / 255) - 0.5) * 2)``
    with numpy float64 inside (shgan_default.py:283, eva_lpips.py:39,43).  'gt': a loader's decoded pixel -- its ``u8_value_table``
    value as ``real`` ('pm1') then ``((real + 1) / 2 - 0.5) * 2``, or ``float32(u8 / 255)`` ('unit') then ``(u - 0.5) * 2``, in float32."""
    if operand == 'pred':
        return torch.from_numpy((((np.arange(256, dtype=np.float64) / 255) - 0.5) * 2).astype(np.float32))
    if gt_range == 'pm1':
        u = (kernels.u8_value_table('cpu') + 1) / 2
    else:
        u = torch.from_numpy((np.arange(256, dtype=np.float64) / 255).astype(np.float32))
    return (u - 0.5) * 2


_LUTS = {}


def value_table(device, operand, gt_range='pm1'):
    key = (str(device), operand, gt_range if operand == 'gt' else None)
    if key not in _LUTS:
        _LUTS[key] = value_table_cpu(operand, gt_range).to(device)
    return _LUTS[key]


def _operand(L, images, operand, gt_range):
    """The operand half of ``conv1`` and ``scaling``: the forms of ``Lpips.__call__`` -> (x, lut, scale, bias) for the call ``L``."""
    if operand not in ('pred', 'gt') or gt_range not in ('pm1', 'unit'):
        raise ShgError(f"lpips: operand must be 'pred' or 'gt' and gt_range 'pm1' or 'unit' (got {operand!r}, {gt_range!r})")
    return kernels._image_operand(L, images, operand, lambda dev: value_table(dev, operand, gt_range),
                                  (0.5, 0.5) if (operand == 'gt' and gt_range == 'pm1') else (1.0, 0.0), 'lpips')


def pack_conv1(w, b):
    """float32 w [64,3,11,11], b [64] on the device -> (wp [368*64], bp [64]) in shg_lpips_conv1_f32's operand layout: that of
    ``inception.pack_weight``, whose entry point stops at the 7 x 7 kernels its convolution serves."""
    L = kernels._Launch()
    w, b = L.req(w, 'w'), L.req(b, 'bias')
    if tuple(w.shape) != (64, 3, 11, 11) or tuple(b.shape) != (64,):
        raise ShgError(f'lpips: conv1 weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected (64, 3, 11, 11) / (64,)')
    wp, bp = L.new((368 * 64,)), L.new((64,))
    with L:
        check(_lib.get_lib().shg_lpips_conv1_weight_prep_f32(kernels._ptr(w), kernels._ptr(b), kernels._ptr(wp), kernels._ptr(bp), L.stream()),
              'lpips_conv1_weight_prep')
    return wp, bp


def conv1(images, wp, bp, operand='pred', gt_range='pm1', shift=SHIFT, scale=SCALE, y=None):
    """images [B,3,H,W] (uint8 or float32, forms of ``Lpips.__call__``) -> relu(conv1(scaling_layer(value))) [B,64,OH,OW] (one launch);
    ``y``: a contiguous float32 [B,64,OH,OW] view to write into."""
    L = kernels._Launch()
    x, lut, s, b = _operand(L, images, operand, gt_range)
    wp, bp = L.req(wp, 'wp'), L.req(bp, 'bp')
    B, _, H, W = x.shape
    if H < 7 or W < 7:
        raise ShgError(f'lpips: conv1 needs H, W >= 7 (got {H} x {W})')
    OH, OW = inception.out_size(H, 11, 4, 2), inception.out_size(W, 11, 4, 2)
    if y is None:
        y = L.new((B, 64, OH, OW))
    L.view(y, 'y')
    if tuple(y.shape) != (B, 64, OH, OW) or not y.is_contiguous() or y.dtype != torch.float32 or not y.is_cuda:
        raise ShgError(f'lpips: conv1 output {tuple(y.shape)} does not fit input {tuple(x.shape)}')
    with L:
        check(_lib.get_lib().shg_lpips_conv1_f32(kernels._ptr(x), kernels._ptr(lut), s, b, kernels._c3(shift), kernels._c3(scale),
                                                 kernels._ptr(wp), kernels._ptr(bp), kernels._ptr(y), B, H, W, L.stream()), 'lpips_conv1')
    return y


def scaling(images, operand='pred', gt_range='pm1', shift=SHIFT, scale=SCALE, y=None):
    """images [B,3,H,W] (uint8 or float32, forms of ``Lpips.__call__``) -> scaling_layer(value) [B,3,H,W] float32, the float32 steps of
    conv1's load (one launch); ``y``: a contiguous float32 [B,3,H,W] view to write into."""
    L = kernels._Launch()
    x, lut, s, b = _operand(L, images, operand, gt_range)
    if y is None:
        y = L.new(tuple(x.shape))
    L.view(y, 'y')
    if tuple(y.shape) != tuple(x.shape) or not y.is_contiguous() or y.dtype != torch.float32 or not y.is_cuda:
        raise ShgError(f'lpips: scaling output {tuple(y.shape)} does not fit input {tuple(x.shape)}')
    B, _, H, W = x.shape
    with L:
        check(_lib.get_lib().shg_lpips_scaling_f32(kernels._ptr(x), kernels._ptr(lut), s, b, kernels._c3(shift), kernels._c3(scale),
                                                   kernels._ptr(y), B, H, W, L.stream()), 'lpips_scaling')
    return y


def head(fp, fg, w, out):
    """One tap: fp, fg [B,C,h,w] float32 (features of the preds / the gts), w [C] -> out [B] float64 += spatial mean of d."""
    L = kernels._Launch()
    fp, fg, w = L.req(fp, 'fp'), L.req(fg, 'fg'), L.req(w, 'w')
    L.req(out, 'out', dtype=torch.float64)
    if fp.ndim != 4 or tuple(fp.shape) != tuple(fg.shape) or w.numel() != fp.shape[1]:
        raise ShgError(f'lpips: head operands {tuple(fp.shape)}, {tuple(fg.shape)}, w {tuple(w.shape)} do not fit')
    B, C, h, wd = fp.shape
    if out.numel() != B or not out.is_contiguous():
        raise ShgError(f'lpips: out must be a contiguous float64 [{B}] tensor')
    lib = _lib.get_lib()
    nbytes = int(lib.shg_lpips_head_scratch_bytes(B, h, wd))
    scratch = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=L.dev)
    with L:
        check(lib.shg_lpips_head_f32(kernels._ptr(fp), kernels._ptr(fg), kernels._ptr(w), B, C, h, wd, kernels._ptr(scratch), nbytes,
                                     kernels._ptr(out), L.stream()), 'lpips_head')
    return out


def head_pairs(f, ia, ib, w, out, err=None):
    """One tap, pair form: f [M,C,h,w] float32, ia / ib int32 [P] (rows of f), w [C] -> out [P] float64 += the head's value of the pair
    (f[ia[p]], f[ib[p]]): the bits of ``head(f[ia], f[ib], w, out)``, whatever P and the pair's place in the table.  Tables on the CPU are
    checked on the host (an index outside [0, M) raises ShgError and nothing is launched) and copied to the device; tables that are already
    HIP tensors are not read by the host: the kernel clamps an index into [0, M) and stores 1 into ``err`` (int32 [1] HIP tensor, zeroed by
    the caller; optional)."""
    launch = kernels._Launch()               # (``launch``, not ``L``: see the note above kernels.plural_composite_u8)
    f, w = launch.req(f, 'f'), launch.req(w, 'w')
    launch.req(out, 'out', dtype=torch.float64)
    if f.ndim != 4 or w.numel() != f.shape[1]:
        raise ShgError(f'lpips: head_pairs operands f {tuple(f.shape)}, w {tuple(w.shape)} do not fit')
    for name, t in (('ia', ia), ('ib', ib)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.ndim != 1 or t.numel() != ia.numel() or t.is_cuda != ia.is_cuda:
            raise ShgError(f'lpips: head_pairs {name} must be an int32 [P] tensor, both tables on the same side')
    M, C, h, wd = f.shape
    P = ia.numel()
    if P < 1 or out.numel() != P or not out.is_contiguous():
        raise ShgError(f'lpips: out must be a contiguous float64 [{P}] tensor, P >= 1')
    host = (None, None)
    if not ia.is_cuda:
        ia, ib = ia.contiguous(), ib.contiguous()
        host = tuple(ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int)) for t in (ia, ib))
        ia_d, ib_d = ia.to(launch.dev), ib.to(launch.dev)
    else:
        ia_d, ib_d = launch.req(ia, 'ia', dtype=torch.int32), launch.req(ib, 'ib', dtype=torch.int32)
    if err is not None:
        launch.req(err, 'err', dtype=torch.int32)
    lib = _lib.get_lib()
    nbytes = int(lib.shg_lpips_head_pairs_scratch_bytes(P, h, wd))
    scratch = launch.new((max(1, nbytes // 8),), torch.float64)
    with launch:
        check(lib.shg_lpips_head_pairs_f32(kernels._ptr(f), kernels._ptr(ia_d), kernels._ptr(ib_d), host[0], host[1], kernels._ptr(w), M, P, C, h, wd,
                                           kernels._ptr(scratch), nbytes, kernels._ptr(out), kernels._ptr(err), launch.stream()), 'lpips_head_pairs')
    return out


# ---- the training loss: operands in [-1, 1] straight into the scaling layer, and the backward pass with respect to the pred image
# (csrc/lpips_bwd.hip).  ONE masking rule: whoever writes a gradient into the buffer of a post-ReLU activation y selects it by y > 0.
# (``launch``, not ``L``, in these functions: see the note above kernels.plural_composite_u8 -- the allocation tables of
# tests/test_gpu_alloc_fill.py and tests/test_gpu_alloc_guard.py are older than they are.)

def _pm1(launch, x, name='x'):
    x = launch.req(x, name)
    if x.ndim != 4 or x.shape[1] != 3:
        raise ShgError(f'lpips: {name} must be a float32 [B,3,H,W] tensor (got {tuple(x.shape)})')
    return x


def scale_pm1(x, shift=SHIFT, scale=SCALE):
    """x [B,3,H,W] float32 in [-1, 1] -> scaling_layer(x) = (x - shift_c) * float32(1 / scale_c) (one launch)."""
    launch = kernels._Launch()
    x = _pm1(launch, x)
    B, _, H, W = x.shape
    y = launch.new(tuple(x.shape))
    with launch:
        check(_lib.get_lib().shg_lpips_scale_pm1_f32(kernels._ptr(x), kernels._c3(shift), kernels._c3(scale), kernels._ptr(y), B, H, W, launch.stream()),
              'lpips_scale_pm1')
    return y


def conv1_pm1(x, wp, bp, shift=SHIFT, scale=SCALE):
    """x [B,3,H,W] float32 in [-1, 1] -> relu(conv1(scaling_layer(x))) [B,64,OH,OW] (one launch): ``conv1`` with the plain operand."""
    launch = kernels._Launch()
    x, wp, bp = _pm1(launch, x), launch.req(wp, 'wp'), launch.req(bp, 'bp')
    B, _, H, W = x.shape
    if H < 7 or W < 7:
        raise ShgError(f'lpips: conv1 needs H, W >= 7 (got {H} x {W})')
    y = launch.new((B, 64, inception.out_size(H, 11, 4, 2), inception.out_size(W, 11, 4, 2)))
    with launch:
        check(_lib.get_lib().shg_lpips_conv1_pm1_f32(kernels._ptr(x), kernels._c3(shift), kernels._c3(scale), kernels._ptr(wp), kernels._ptr(bp),
                                                     kernels._ptr(y), B, H, W, launch.stream()), 'lpips_conv1_pm1')
    return y


def unpack_weight(wp, O, I, kh, kw):
    """The inverse of ``inception.pack_weight``: wp [Kp*Np] -> w [O,I,kh,kw] (a torch view + copy; once per network)."""
    Np = (O + 63) // 64 * 64
    return wp.reshape(-1, Np)[:I * kh * kw, :O].reshape(kh, kw, I, O).permute(3, 2, 0, 1).contiguous()


def pack_dgrad_weight(w, fold=None):
    """Forward weight w [O,I,k,k] on the device -> the packed operand of ``dgrad``: ``w.transpose(0,1).flip(2,3)`` [I,O,k,k] through
    ``inception.pack_weight``.  ``fold`` [I]: a factor per INPUT channel of the forward convolution (the scaling layer's 1 / scale_c)."""
    wt = w.transpose(0, 1).flip(2, 3)
    if fold is not None:
        wt = wt * fold.to(wt).reshape(-1, 1, 1, 1)
    wt = wt.contiguous()
    return inception.pack_weight(wt, wt[:, 0, 0, 0].contiguous())[0]      # (the packing wants a bias [O]; dgrad has none and drops it)


def dgrad(g, wp, O, k, ymask=None):
    """Input gradient of a stride-1 k x k convolution at pad k // 2: g [B,I,H,W], wp = ``pack_dgrad_weight(w)`` -> dx [B,O,H,W], selected
    by ``ymask > 0`` (a [B,O,H,W] post-ReLU activation) when given (one launch on the detector's tile, K never split)."""
    launch = kernels._Launch()
    g, wp, ymask = launch.req(g, 'g'), launch.req(wp, 'wp'), launch.req(ymask, 'ymask')
    if g.ndim != 4:
        raise ShgError(f'lpips: dgrad takes g [B,I,H,W] (got {tuple(g.shape)})')
    B, I, H, W = g.shape
    n = int(_lib.get_lib().shg_inception_packed_weight_elems(O, I, k, k))
    if n <= 0 or wp.numel() != n:
        raise ShgError(f'lpips: dgrad weight of {wp.numel()} elements does not fit O {O} I {I} {k}x{k}')
    if ymask is not None and tuple(ymask.shape) != (B, O, H, W):
        raise ShgError(f'lpips: dgrad ymask {tuple(ymask.shape)} does not fit the output {(B, O, H, W)}')
    dx = launch.new((B, O, H, W))
    with launch:
        check(_lib.get_lib().shg_lpips_dgrad_f32(kernels._ptr(g), kernels._ptr(wp), kernels._ptr(ymask), kernels._ptr(dx), B, I, O, H, W, k, k // 2,
                                                 launch.stream()), 'lpips_dgrad')
    return dx


def maxpool_bwd(x, gy, k):
    """Backward of the k x k / stride 2 / floor max pool (k = 2 or 3) of the post-ReLU activation x [B,C,H,W], gather form: gy [B,C,OH,OW]
    -> dx [B,C,H,W] = x > 0 ? the gradients of the windows whose first maximum (row-major) the element is : 0 (one launch)."""
    launch = kernels._Launch()
    x, gy = launch.req(x, 'x'), launch.req(gy, 'gy')
    if x.ndim != 4 or k not in (2, 3) or min(x.shape[2:]) < k or tuple(gy.shape) != tuple(x.shape[:2]) + ((x.shape[2] - k) // 2 + 1, (x.shape[3] - k) // 2 + 1):
        raise ShgError(f'lpips: maxpool_bwd operands x {tuple(x.shape)}, gy {tuple(gy.shape)}, window {k} do not fit')
    B, C, H, W = x.shape
    dx = launch.new(tuple(x.shape))
    with launch:
        check(_lib.get_lib().shg_lpips_maxpool_bwd_f32(kernels._ptr(x), kernels._ptr(gy), kernels._ptr(dx), B, C, H, W, k, launch.stream()), 'lpips_maxpool_bwd')
    return dx


def head_bwd(f, fr, w, g, df=None):
    """One tap's head backward: f, fr [B,C,h,w] (pred / real tap), w [C], g [B] float32 -> df [B,C,h,w], selected by f > 0.  ``df`` given:
    accumulated into it (a tap whose buffer its downstream consumer has written); else a new tensor (one launch)."""
    launch = kernels._Launch()
    f, fr, w, g = launch.req(f, 'f'), launch.req(fr, 'fr'), launch.req(w, 'w'), launch.req(g, 'g')
    if f.ndim != 4 or tuple(f.shape) != tuple(fr.shape) or w.numel() != f.shape[1] or g.numel() != f.shape[0]:
        raise ShgError(f'lpips: head_bwd operands {tuple(f.shape)}, {tuple(fr.shape)}, w {tuple(w.shape)}, g {tuple(g.shape)} do not fit')
    acc = df is not None
    if acc:
        launch.req(df, 'df')
        if tuple(df.shape) != tuple(f.shape) or not df.is_contiguous():
            raise ShgError(f'lpips: head_bwd df {tuple(df.shape)} must be a contiguous tensor of the shape of f {tuple(f.shape)}')
    else:
        df = launch.new(tuple(f.shape))
    B, C, h, wd = f.shape
    with launch:
        check(_lib.get_lib().shg_lpips_head_bwd_f32(kernels._ptr(f), kernels._ptr(fr), kernels._ptr(w), kernels._ptr(g), kernels._ptr(df), B, C, h, wd,
                                                    int(acc), launch.stream()), 'lpips_head_bwd')
    return df


def conv1_dgrad(g, w, H, W):
    """AlexNet conv1's input gradient: g [B,64,OH,OW], w [64,3,11,11] (1 / scale_c folded in) -> dx [B,3,H,W]; the transposed 11 x 11
    stride 4 pad 2 convolution, 0 at the pixels no window reaches (one launch)."""
    launch = kernels._Launch()
    g, w = launch.req(g, 'g'), launch.req(w, 'w')
    if g.ndim != 4 or tuple(g.shape[1:]) != (64, inception.out_size(H, 11, 4, 2), inception.out_size(W, 11, 4, 2)) or tuple(w.shape) != (64, 3, 11, 11):
        raise ShgError(f'lpips: conv1_dgrad operands g {tuple(g.shape)}, w {tuple(w.shape)} do not fit an image of {H} x {W}')
    dx = launch.new((g.shape[0], 3, H, W))
    with launch:
        check(_lib.get_lib().shg_lpips_conv1_dgrad_f32(kernels._ptr(g), kernels._ptr(w), kernels._ptr(dx), g.shape[0], H, W, launch.stream()), 'lpips_conv1_dgrad')
    return dx


def _conv_relu(op, x):
    """One stride-1 'same' convolution + ReLU of the backbone into a new tensor (``split_k`` off: no launch plan depends on the batch)."""
    launch = kernels._Launch()
    launch.view(x, 'x')
    y = launch.new((x.shape[0], op.O) + tuple(x.shape[2:]))
    inception.conv_group([(op, x, 0, y, 0)], split_k=False)
    return y


class _LpipsLoss(torch.autograd.Function):
    """``Lpips.loss``: the value from the forward heads (float64, rounded once), the gradient with respect to ``fake`` from
    csrc/lpips_bwd.hip.  First order only."""

    @staticmethod
    def forward(ctx, fake, real, net):
        B = fake.shape[0]
        ctx.save_for_backward(fake)
        fake, real = fake.detach(), real.detach()
        real_taps = net._taps_pm1(real)
        acts = net._acts_pm1(fake, keep=ctx.needs_input_grad[0])     # every post-ReLU activation of the pred half, in network order
        launch = kernels._Launch()
        launch.view(fake, 'fake')
        out = launch.new((B,), torch.float64).zero_()
        for k, tr, w in zip(net.tap_ids, real_taps, net.lins):
            head(acts[k], tr, w, out)
        ctx.net, ctx.acts, ctx.real_taps, ctx.size = net, acts, real_taps, tuple(fake.shape[2:])
        return out.to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def _once(ctx, g):
        net, acts, real_taps = ctx.net, ctx.acts, ctx.real_taps
        if acts is None:
            raise ShgError('lpips: the activations Lpips.loss saved were freed by its first backward pass: it cannot run backward a second '
                           'time (retain_graph=True does not keep them)')
        ctx.acts = ctx.real_taps = None
        return net._backward(acts, real_taps, g.to(torch.float32).contiguous(), ctx.size)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return kernels.first_order_only(_LpipsLoss._once(ctx, g), ctx.saved_tensors[0], 'Lpips.loss'), None, None


class Lpips:
    """``net(pred, gt, gt_range='pm1', out=None) -> float64 [B]``.  pred: uint8 composite or float32 in [0, 1]; gt: float32 in [-1, 1] or
    decoded uint8 pixels ('pm1'), or float32 in [0, 1] / uint8 with ``gt_range='unit'`` -- the operand forms of
    ``image_metrics.image_metrics``.  Every launch goes to the current stream and every buffer comes from torch's caching allocator on it,
    so the network runs on any stream (EvalLoop's side streams) concurrently with itself.  ``net(pred_u8, real, out=slice)`` is the
    callable ``EvalLoop(lpips=...)`` takes."""

    def __init__(self, conv1_wb, ops, lins, shift, scale, device, split_k=False, net='alex', mean=vgg16.CAFFE_MEAN, std=(1.0, 1.0, 1.0)):
        if net not in NETS:
            raise ShgError(f'lpips: net must be one of {NETS} (got {net!r})')
        self.conv1_wb, self.ops, self.lins = conv1_wb, ops, lins
        self.shift, self.scale = tuple(float(v) for v in shift), tuple(float(v) for v in scale)
        self.device, self.split_k, self.net = torch.device(device), split_k, net
        self.min_size = MIN_SIZE if net == 'alex' else VGG_MIN_SIZE
        # net='vgg' only: the normalisation of a 0..255 image for ``trunk``'s other caller (ppl.py), in the order the image is read (RGB)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.widths = tuple(op.O for op in ops) if net == 'vgg' else None
        self._dgrad, self.loss_calls = None, 0      # the transposed weights (packed at the first ``loss``); how often ``loss`` ran

    @classmethod
    def _from_canonical(cls, cw, device, split_k):
        dev = torch.device(device)
        conv1_wb = pack_conv1(cw['conv0.weight'].to(dev), cw['conv0.bias'].to(dev))
        ops = []
        for k, (i, o, ks, s, p) in enumerate(CONVS[1:], start=1):
            wp, bp = inception.pack_weight(cw[f'conv{k}.weight'].to(dev), cw[f'conv{k}.bias'].to(dev))
            ops.append(inception.ConvOp(f'conv{k + 1}', wp, bp, i, o, (ks, ks), (s, s), (p, p)))
        lins = [cw[f'lin{k}'].to(dev) for k in range(5)]
        return cls(conv1_wb, ops, lins, cw['shift'].tolist(), cw['scale'].tolist(), dev, split_k)

    @classmethod
    def _from_canonical_vgg(cls, cw, device, mean, std, bgr):
        if len(mean) != 3 or len(std) != 3 or min(float(v) for v in std) <= 0:
            raise ShgError(f'lpips: mean and std must be three numbers each, std positive (got {mean!r}, {std!r})')
        dev = torch.device(device)
        ops = vgg16.conv_ops([(f'vgg.conv{k}', cw[f'conv{k}.weight'], cw[f'conv{k}.bias']) for k in range(len(cw['widths']))], dev, bgr)
        lins = [cw[f'lin{n}'].to(dev) for n in range(5)]
        consts = [cw['shift'].tolist(), cw['scale'].tolist(), tuple(mean), tuple(std)]
        if bgr:
            consts = [tuple(v)[::-1] for v in consts]
        return cls(None, ops, lins, consts[0], consts[1], dev, False, net='vgg', mean=consts[2], std=consts[3])

    @classmethod
    def from_state_dict(cls, sd, device='cuda', split_k=False, net='alex', mean=vgg16.CAFFE_MEAN, std=(1.0, 1.0, 1.0), bgr=False):
        """The package's full ``state_dict`` (``lpips.LPIPS(net=net).state_dict()``).  ``mean``, ``std``, ``bgr``: net='vgg' only."""
        if net not in NETS:
            raise ShgError(f'lpips: net must be one of {NETS} (got {net!r})')
        if net == 'vgg':
            return cls._from_canonical_vgg(canonical_vgg_weights(sd), device, mean, std, bgr)
        return cls._from_canonical(canonical_weights(sd), device, split_k)

    @classmethod
    def from_state_dicts(cls, alexnet_sd, lin_sd, device='cuda', split_k=False, net='alex', mean=vgg16.CAFFE_MEAN, std=(1.0, 1.0, 1.0), bgr=False):
        """torchvision's ``alexnet`` (net='vgg': ``vgg16``) state_dict + the package's ``weights/v0.1/alex.pth`` (``vgg.pth``): the ``lin``
        weights come from a file of their own."""
        if net not in NETS:
            raise ShgError(f'lpips: net must be one of {NETS} (got {net!r})')
        if net == 'vgg':
            return cls._from_canonical_vgg(canonical_vgg_weights(alexnet_sd, lin_sd), device, mean, std, bgr)
        return cls._from_canonical(canonical_weights(alexnet_sd, lin_sd), device, split_k)

    def trunk(self, x):
        """net='vgg': x [N,3,H,W] float32, a finished network input (after the scaling layer, or the path-length front end) -> the five
        taps [N,C,h,w].  No launch plan depends on N."""
        if self.net != 'vgg':
            raise ShgError("lpips: trunk() is the net='vgg' backbone")
        return vgg16.conv_trunk(self.ops, x, taps=VGG_TAPS)

    def features(self, pred, gt, gt_range='pm1'):
        """-> the five taps, each [2B,C,h,w] float32: the preds' features in [:B], the gts' in [B:].  ``gt=None``: the preds alone, [B,C,h,w]."""
        B, _, H, W = pred.shape
        T = B if gt is None else 2 * B
        if self.net == 'vgg':
            x = torch.empty((T, 3, H, W), dtype=torch.float32, device=self.device)
            scaling(pred, 'pred', gt_range, self.shift, self.scale, y=x[:B])
            if gt is not None:
                scaling(gt, 'gt', gt_range, self.shift, self.scale, y=x[B:])
            return self.trunk(x)
        oh, ow = out_sizes(H), out_sizes(W)
        new = lambda k: torch.empty((T, TAP_CHANNELS[k], oh[k], ow[k]), dtype=torch.float32, device=self.device)    # noqa: E731
        t0 = new(0)
        conv1(pred, *self.conv1_wb, 'pred', gt_range, self.shift, self.scale, y=t0[:B])
        if gt is not None:
            conv1(gt, *self.conv1_wb, 'gt', gt_range, self.shift, self.scale, y=t0[B:])
        taps, x = [t0], inception.pool(t0, 'max', 2, 0)
        for k, op in enumerate(self.ops, start=1):
            y = new(k)
            inception.conv_group([(op, x, 0, y, 0)], split_k=self.split_k)
            taps.append(y)
            x = inception.pool(y, 'max', 2, 0) if k == 1 else y
        return taps

    def taps_of(self, images):
        """images [B,3,H,W] in the 'pred' operand form (uint8 composite or float32 in [0, 1]) -> the five taps [B,C,h,w]: ONE pass of the
        backbone over the batch, the launches ``features`` issues for its pred half (no launch plan depends on the batch size)."""
        return self.features(images, None)

    # -- the training loss (first order; csrc/lpips_bwd.hip) ------------------------------------------------------------------------------
    @property
    def tap_ids(self):
        """Index of each tap in the list of post-ReLU activations ``_acts_pm1`` returns."""
        return VGG_TAPS if self.net == 'vgg' else (0, 1, 2, 3, 4)

    def _acts_pm1(self, x, keep=True):
        """x [B,3,H,W] float32 in [-1, 1], straight into the scaling layer -> every post-ReLU activation in network order (vgg: 13, alex:
        5), the saving variant of ``features`` / ``vgg16.conv_trunk``: the same launches, pooled tensors dropped.  ``keep=False``: a
        non-tap activation is dropped as soon as its consumer has read it (None in the list)."""
        acts = []
        if self.net == 'vgg':
            x = scale_pm1(x, self.shift, self.scale)
            for k, op in enumerate(self.ops):
                y = _conv_relu(op, x)
                acts.append(y if keep or k in VGG_TAPS else None)
                x = vgg16.maxpool2(y) if k in vgg16.POOL_AFTER and k + 1 < len(self.ops) else y
            return acts
        y = conv1_pm1(x, *self.conv1_wb, self.shift, self.scale)
        acts.append(y)
        x = inception.pool(y, 'max', 2, 0)
        for k, op in enumerate(self.ops, start=1):
            y = _conv_relu(op, x)
            acts.append(y)
            x = inception.pool(y, 'max', 2, 0) if k == 1 else y
        return acts

    def _taps_pm1(self, x):
        """The real half: the five taps only."""
        acts = self._acts_pm1(x, keep=False)
        return [acts[k] for k in self.tap_ids]

    def _dgrad_weights(self):
        """The transposed weights, packed once per network (from the packed forward operands): [(wp, O, k)] per convolution whose dgrad
        runs on the tile; 1 / scale_c folded into the first (vgg) or into conv1's plain weight (alex: ``_conv1_wt``)."""
        if self._dgrad is None:
            inv = torch.tensor([float(np.float32(1.0 / float(np.float32(s)))) for s in self.scale], dtype=torch.float32, device=self.device)
            packs = []
            for n, op in enumerate(self.ops):
                w = unpack_weight(op.wp, op.O, op.I, op.k[0], op.k[1])
                packs.append((pack_dgrad_weight(w, inv if (self.net == 'vgg' and n == 0) else None), op.I, op.k[0]))
            if self.net == 'alex':
                self._conv1_wt = (unpack_weight(self.conv1_wb[0], 64, 3, 11, 11) * inv.reshape(1, 3, 1, 1)).contiguous()
            self._dgrad = packs
        return self._dgrad

    def _backward(self, acts, real_taps, g, size):
        """g [B] float32 -> d(sum_b g_b loss_b) / d fake [B,3,H,W].  Every activation gradient is written once -- by the dgrad or the pool
        backward downstream of it, which selects by y > 0 -- accumulated into once by the head where it is a tap, and read once."""
        packs = self._dgrad_weights()
        taps = {k: n for n, k in enumerate(self.tap_ids)}
        last = len(acts) - 1
        gy = head_bwd(acts[last], real_taps[4], self.lins[4], g)
        if self.net == 'vgg':
            for k in range(last, 0, -1):
                wp, O, ks = packs[k]
                pooled = (k - 1) in vgg16.POOL_AFTER
                gy = dgrad(gy, wp, O, ks, None if pooled else acts[k - 1])
                if pooled:
                    gy = maxpool_bwd(acts[k - 1], gy, 2)
                if (k - 1) in taps:
                    head_bwd(acts[k - 1], real_taps[taps[k - 1]], self.lins[taps[k - 1]], g, df=gy)
                acts[k] = None
            wp, O, ks = packs[0]
            return dgrad(gy, wp, O, ks, None)
        for k in range(4, 0, -1):                                    # acts[k] is the output of self.ops[k - 1]
            wp, O, ks = packs[k - 1]
            pooled = k <= 2
            gy = dgrad(gy, wp, O, ks, None if pooled else acts[k - 1])
            if pooled:
                gy = maxpool_bwd(acts[k - 1], gy, 3)
            head_bwd(acts[k - 1], real_taps[k - 1], self.lins[k - 1], g, df=gy)
            acts[k] = None
        return conv1_dgrad(gy, self._conv1_wt, size[0], size[1])

    def _check_pair(self, a, b, names):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.ndim != 4 or tuple(a.shape) != tuple(b.shape) or a.shape[1] != 3:
            raise ShgError(f'lpips: {names[0]} and {names[1]} must be [B,3,H,W] tensors of one shape')
        if not (a.is_cuda and b.is_cuda):
            raise ShgError(f'lpips: {names[0]} and {names[1]} must reside on a HIP (cuda) device: there is no CPU path')
        H, W = a.shape[2:]
        if H < self.min_size or W < self.min_size:
            why = 'the AlexNet taps need H, W >= 31 (the second max pool must see 3 x 3)' if self.net == 'alex' else \
                'the VGG16 taps need H, W >= 16 (four 2 x 2 pools before the last one)'
            raise ShgError(f'lpips: images of {H} x {W} are too small: {why}')

    def loss(self, fake, real):
        """The distance as a training loss: ``fake``, ``real`` float32 [B,3,H,W] in [-1, 1] on the device -> float32 [B], the distance
        ``__call__`` computes (accumulated in float64, rounded once) except that both operands enter the scaling layer ``(v - shift) /
        scale`` as they are.  ``fake`` may require grad; ``real`` never gets a gradient.  First order only: a second derivative raises.
        The pred half keeps every post-ReLU activation until backward, the real half only its taps.  ``split_k`` is off on this route."""
        self._check_pair(fake, real, ('fake', 'real'))
        if fake.dtype != torch.float32 or real.dtype != torch.float32:
            raise ShgError(f'lpips: loss takes float32 images in [-1, 1] (got {fake.dtype}, {real.dtype})')
        self.loss_calls += 1
        self._dgrad_weights()
        return _LpipsLoss.apply(fake, real, self)

    def __call__(self, pred, gt, gt_range='pm1', out=None):
        if gt_range not in ('pm1', 'unit'):
            raise ShgError(f"lpips: gt_range must be 'pm1' or 'unit' (got {gt_range!r})")
        if not (isinstance(pred, torch.Tensor) and isinstance(gt, torch.Tensor)) or pred.ndim != 4 or tuple(pred.shape) != tuple(gt.shape) \
                or pred.shape[1] != 3:
            raise ShgError('lpips: pred and gt must be [B,3,H,W] tensors of one shape')
        if not (pred.is_cuda and gt.is_cuda):
            raise ShgError('lpips: pred and gt must reside on a HIP (cuda) device: there is no CPU path')
        B, _, H, W = pred.shape
        if H < self.min_size or W < self.min_size:
            why = 'the AlexNet taps need H, W >= 31 (the second max pool must see 3 x 3)' if self.net == 'alex' else \
                'the VGG16 taps need H, W >= 16 (four 2 x 2 pools before the last one)'
            raise ShgError(f'lpips: images of {H} x {W} are too small: {why}')
        with torch.no_grad():
            if out is None:
                out = torch.zeros(B, dtype=torch.float64, device=self.device)
            else:
                if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (B,) or not out.is_contiguous():
                    raise ShgError(f'lpips: out must be a contiguous float64 [{B}] tensor')
                out.zero_()
            for t, w in zip(self.features(pred, gt, gt_range), self.lins):
                head(t[:B], t[B:], w, out)
        return out


def LPIPS(net='alex', state_dict=None, lin_state_dict=None, device='cuda', **options):
    """The package's constructor form: ``LPIPS(net='alex' | 'vgg', state_dict=full_sd)`` or ``LPIPS(net=..., state_dict=backbone_sd,
    lin_state_dict=lin_sd)`` -> ``Lpips``.  The weights are downloads and are not shipped: a call without them raises.  ``options``:
    ``split_k`` (alex), ``mean`` / ``std`` / ``bgr`` (vgg)."""
    if net not in NETS:
        raise ShgError(f'lpips: net must be one of {NETS} (got {net!r})')
    if state_dict is None:
        raise ShgError(f'lpips: LPIPS(net={net!r}) needs state_dict=...: the weights are downloads and are not shipped')
    if lin_state_dict is None:
        return Lpips.from_state_dict(state_dict, device=device, net=net, **options)
    return Lpips.from_state_dicts(state_dict, lin_state_dict, device=device, net=net, **options)
