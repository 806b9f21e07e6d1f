"""The FID detector: the feature extractor of Inception-v3 ``inception-2015-12-05`` (the TF graph the reference's eva_fid.py:30,145-158
loads as a TorchScript download), on the HIP kernels of csrc/inception.hip.

    det = InceptionFeatures.from_state_dict(torch.load('pt_inception-2015-12-05-6726825d.pth'), device='cuda')
    feats = det(images, return_features=True)                    # [B, 2048] float32, on the current stream

``images`` [B,3,H,W] of any size: uint8 (the composite ``EvalLoop`` holds; value = the byte) or float32 in 0..255 (what
``FidStats.add_images`` hands over); ``input_range='pm1'`` takes the loop's ``real`` instead -- float32 in [-1, 1] mapped as the
reference does (``real.float()*127.5 + 127.5`` in float32), or a loader's decoded uint8 pixels through ``kernels.u8_value_table`` first.

Front end (one launch): TF1's legacy bilinear resize to 299 x 299 -- source coordinate ``i * W / 299``, no half-pixel offset, border
samples clamped; skipped at 299 x 299 -- then ``(x - 128) / 128``.  This follows the published forward of the reference's detector
(``affine_grid`` with a shifted theta + ``grid_sample(bilinear, padding_mode='border', align_corners=False)``, which is the same mapping);
it was NOT checked against the detector file itself, which is a download.

Body: the FID variant of Inception-v3 (pytorch-fid's ``FIDInception*`` blocks): stem, Mixed_5b-5d, 6a, 6b-6e, 7a, 7b, 7c, global
average pool -> 2048; every convolution is followed by BatchNorm (eps 1e-3) and ReLU; the pool branches of the A, C and Mixed_7b blocks
average over the in-bounds taps (``count_include_pad=False``), Mixed_7c's pool branch is a 3 x 3 max pool; branches are concatenated in
torchvision order.  The classifier head (``fc.weight`` [C, 2048], ``fc.bias`` [C]) is optional: with it ``return_features=False`` gives
the softmax probabilities [B, C] the Inception Score needs (one more launch on the pooled features; C = 1008 for the 2015 graph, 1000 for a
torchvision file); without it that call raises.

Weights: a ``state_dict`` in the torchvision / pytorch-fid key layout (``Conv2d_1a_3x3.conv.weight``, ``Conv2d_1a_3x3.bn.{weight, bias,
running_mean, running_var}``, ..., ``Mixed_7c.branch_pool.*``; ``AuxLogits.*`` is ignored, ``fc.*`` is the optional head,
``bn.num_batches_tracked`` is accepted).  This is the layout of pytorch-fid's ``pt_inception-2015-12-05-*.pth`` port of the TF weights; it was not checked against
that file here, and neither was the head's key name (``fc``; the TorchScript detector may call its last layer otherwise).  BatchNorm is folded into the convolution weight and a per-channel bias once, on the host in float64."""
import collections

import torch

from . import _lib, kernels
from ._lib import ShgError, check

RES = 299
DIM = 2048
BN_EPS = 1e-3


def _spec():
    """name -> (I, O, (kh, kw), (sh, sw), (ph, pw), input size) of all 94 convolutions, in network order."""
    L = collections.OrderedDict()

    def add(name, i, o, k, s=1, p=0, h=None):
        k = (k, k) if isinstance(k, int) else k
        s = (s, s) if isinstance(s, int) else s
        p = (p, p) if isinstance(p, int) else p
        L[name] = (i, o, k, s, p, h)
    add('Conv2d_1a_3x3', 3, 32, 3, 2, h=299)
    add('Conv2d_2a_3x3', 32, 32, 3, h=149)
    add('Conv2d_2b_3x3', 32, 64, 3, p=1, h=147)
    add('Conv2d_3b_1x1', 64, 80, 1, h=73)
    add('Conv2d_4a_3x3', 80, 192, 3, h=73)
    for name, cin, pf in (('Mixed_5b', 192, 32), ('Mixed_5c', 256, 64), ('Mixed_5d', 288, 64)):
        add(f'{name}.branch1x1', cin, 64, 1, h=35)
        add(f'{name}.branch5x5_1', cin, 48, 1, h=35)
        add(f'{name}.branch5x5_2', 48, 64, 5, p=2, h=35)
        add(f'{name}.branch3x3dbl_1', cin, 64, 1, h=35)
        add(f'{name}.branch3x3dbl_2', 64, 96, 3, p=1, h=35)
        add(f'{name}.branch3x3dbl_3', 96, 96, 3, p=1, h=35)
        add(f'{name}.branch_pool', cin, pf, 1, h=35)
    add('Mixed_6a.branch3x3', 288, 384, 3, 2, h=35)
    add('Mixed_6a.branch3x3dbl_1', 288, 64, 1, h=35)
    add('Mixed_6a.branch3x3dbl_2', 64, 96, 3, p=1, h=35)
    add('Mixed_6a.branch3x3dbl_3', 96, 96, 3, 2, h=35)
    for name, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
        add(f'{name}.branch1x1', 768, 192, 1, h=17)
        add(f'{name}.branch7x7_1', 768, c7, 1, h=17)
        add(f'{name}.branch7x7_2', c7, c7, (1, 7), p=(0, 3), h=17)
        add(f'{name}.branch7x7_3', c7, 192, (7, 1), p=(3, 0), h=17)
        add(f'{name}.branch7x7dbl_1', 768, c7, 1, h=17)
        add(f'{name}.branch7x7dbl_2', c7, c7, (7, 1), p=(3, 0), h=17)
        add(f'{name}.branch7x7dbl_3', c7, c7, (1, 7), p=(0, 3), h=17)
        add(f'{name}.branch7x7dbl_4', c7, c7, (7, 1), p=(3, 0), h=17)
        add(f'{name}.branch7x7dbl_5', c7, 192, (1, 7), p=(0, 3), h=17)
        add(f'{name}.branch_pool', 768, 192, 1, h=17)
    add('Mixed_7a.branch3x3_1', 768, 192, 1, h=17)
    add('Mixed_7a.branch3x3_2', 192, 320, 3, 2, h=17)
    add('Mixed_7a.branch7x7x3_1', 768, 192, 1, h=17)
    add('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7), p=(0, 3), h=17)
    add('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1), p=(3, 0), h=17)
    add('Mixed_7a.branch7x7x3_4', 192, 192, 3, 2, h=17)
    for name, cin in (('Mixed_7b', 1280), ('Mixed_7c', 2048)):
        add(f'{name}.branch1x1', cin, 320, 1, h=8)
        add(f'{name}.branch3x3_1', cin, 384, 1, h=8)
        add(f'{name}.branch3x3_2a', 384, 384, (1, 3), p=(0, 1), h=8)
        add(f'{name}.branch3x3_2b', 384, 384, (3, 1), p=(1, 0), h=8)
        add(f'{name}.branch3x3dbl_1', cin, 448, 1, h=8)
        add(f'{name}.branch3x3dbl_2', 448, 384, 3, p=1, h=8)
        add(f'{name}.branch3x3dbl_3a', 384, 384, (1, 3), p=(0, 1), h=8)
        add(f'{name}.branch3x3dbl_3b', 384, 384, (3, 1), p=(1, 0), h=8)
        add(f'{name}.branch_pool', cin, 192, 1, h=8)
    return L


LAYERS = _spec()
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')
IGNORED_PREFIXES = ('fc.', 'AuxLogits.')
HEAD_WEIGHT, HEAD_BIAS = 'fc.weight', 'fc.bias'      # the classifier head (optional; probabilities need it)


def out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def expected_shapes(head_classes=None):
    """state_dict key -> shape of every tensor the detector reads (``bn.num_batches_tracked`` is optional); with ``head_classes`` = C
    also the classifier head's ``fc.weight`` [C, 2048] and ``fc.bias`` [C]."""
    shapes = collections.OrderedDict()
    for name, (i, o, (kh, kw), _, _, _) in LAYERS.items():
        shapes[f'{name}.conv.weight'] = (o, i, kh, kw)
        for k in BN_KEYS:
            shapes[f'{name}.bn.{k}'] = (o,)
    if head_classes is not None:
        shapes[HEAD_WEIGHT] = (int(head_classes), DIM)
        shapes[HEAD_BIAS] = (int(head_classes),)
    return shapes


def validate_state_dict(sd, head=False):
    """Raises ShgError naming the first missing key, unexpected key or wrong shape.  ``head=True`` also asks for the classifier head:
    ``fc.weight`` [C, 2048] with any C >= 1 and ``fc.bias`` [C] (without it ``fc.*`` is ignored, whatever it holds)."""
    want = expected_shapes()
    if head:
        if HEAD_WEIGHT not in sd:
            raise ShgError(f'inception: state_dict lacks {HEAD_WEIGHT!r} (the classifier head)')
        w = sd[HEAD_WEIGHT]
        if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] != DIM:
            raise ShgError(f'inception: {HEAD_WEIGHT!r} has shape {tuple(w.shape)}, expected (C, {DIM})')
        if HEAD_BIAS not in sd:
            raise ShgError(f'inception: state_dict lacks {HEAD_BIAS!r} (the classifier head)')
        if tuple(sd[HEAD_BIAS].shape) != (w.shape[0],):
            raise ShgError(f'inception: {HEAD_BIAS!r} has shape {tuple(sd[HEAD_BIAS].shape)}, expected {(w.shape[0],)}')
    for key in want:
        if key not in sd:
            raise ShgError(f'inception: state_dict lacks {key!r}')
    for key, t in sd.items():
        if key.startswith(IGNORED_PREFIXES):
            continue
        if key.endswith('.bn.num_batches_tracked') and key[:-len('.bn.num_batches_tracked')] in LAYERS:
            continue
        if key not in want:
            raise ShgError(f'inception: unexpected state_dict key {key!r}')
        if tuple(t.shape) != want[key]:
            raise ShgError(f'inception: {key!r} has shape {tuple(t.shape)}, expected {want[key]}')


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) -> BatchNorm(eval) as one conv with bias, in float64: w' = w * gamma / sqrt(var + eps), b' = beta - mean * that."""
    w, gamma, beta, mean, var = (torch.as_tensor(t).detach().cpu().to(torch.float64) for t in (w, gamma, beta, mean, var))
    scale = gamma / torch.sqrt(var + eps)
    return w * scale[:, None, None, None], beta - mean * scale


IncConv = _lib.IncConv
MAX_GROUPS = 8
SPLIT_TARGET = 256          # workgroups a launch should reach before K is split (one per CU)


def pack_weight(w, b):
    """Folded float32 w [O,I,kh,kw], b [O] on the device -> (wp [Kp*Np], bp [Np]) in the conv kernel's operand layout."""
    L = kernels._Launch()
    w = L.req(w, 'w')
    b = L.req(b, 'bias')
    o, i, kh, kw = w.shape
    n = int(_lib.get_lib().shg_inception_packed_weight_elems(o, i, kh, kw))
    if n <= 0:
        raise ShgError(f'inception: bad weight shape {tuple(w.shape)}')
    wp = L.new((n,))
    bp = L.new(((o + 63) // 64 * 64,))
    with L:
        check(_lib.get_lib().shg_inception_weight_prep_f32(kernels._ptr(w), kernels._ptr(b), kernels._ptr(wp), kernels._ptr(bp), o, i, kh, kw,
                                                           L.stream()), 'inception_weight_prep')
    return wp, bp


class ConvOp:
    """One convolution of the detector: packed weight + bias and its geometry (kernel, stride, padding)."""

    def __init__(self, name, wp, bp, I, O, k, s, p):
        self.name, self.wp, self.bp = name, wp, bp
        self.I, self.O, self.k, self.s, self.p = I, O, k, s, p

    def desc(self, x, y, x_coff=0, y_coff=0, splitk=1):
        B, xc, H, W = x.shape
        OH, OW = out_size(H, self.k[0], self.s[0], self.p[0]), out_size(W, self.k[1], self.s[1], self.p[1])
        if y.shape[0] != B or tuple(y.shape[2:]) != (OH, OW):
            raise ShgError(f'inception: {self.name}: output {tuple(y.shape)} does not fit input {tuple(x.shape)}')
        return IncConv(x.data_ptr(), self.wp.data_ptr(), self.bp.data_ptr(), y.data_ptr(), self.I, H, W, xc, x_coff, self.O,
                       self.k[0], self.k[1], self.s[0], self.s[1], self.p[0], self.p[1], OH, OW, y.shape[1], y_coff, splitk)

    def tiles(self, B, H, W):
        OH, OW = out_size(H, self.k[0], self.s[0], self.p[0]), out_size(W, self.k[1], self.s[1], self.p[1])
        return -(-B * OH * OW // 64) * -(-self.O // 64)

    def ksteps(self):
        return -(-self.I * self.k[0] * self.k[1] // 16)


def conv_group(items, split_k=True):
    """One grouped launch of independent convolutions: items = [(ConvOp, x, x_coff, y, y_coff)], all of one batch size, on the
    current stream.  With ``split_k`` a launch of fewer than SPLIT_TARGET workgroups splits the K of its long-K groups (the split
    then depends on the batch size; the sums differ from the unsplit ones by rounding only)."""
    if not 1 <= len(items) <= MAX_GROUPS:
        raise ShgError(f'inception: 1..{MAX_GROUPS} convolutions per launch')
    L = kernels._Launch()
    B = items[0][1].shape[0]
    total = 0
    for op, x, _, y, _ in items:
        for t, what in ((x, 'x'), (y, 'y')):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.ndim != 4:
                raise ShgError(f'inception: {op.name}: {what} must be a contiguous float32 [B,C,H,W] tensor on a HIP device')
            L.view(t, f'{op.name}.{what}')
        if x.shape[0] != B:
            raise ShgError('inception: the convolutions of one launch share the batch size')
        total += op.tiles(B, x.shape[2], x.shape[3])
    descs = []
    for op, x, xo, y, yo in items:
        sk = 1
        if split_k and total < SPLIT_TARGET:
            sk = max(1, min(8, SPLIT_TARGET // total, op.ksteps() // 8))
        descs.append(op.desc(x, y, xo, yo, sk))
    arr = (IncConv * len(descs))(*descs)
    lib = _lib.get_lib()
    nbytes = int(lib.shg_inception_conv_workspace_bytes(arr, len(descs), B))
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=L.dev) if nbytes else None
    with L:
        check(lib.shg_inception_conv_f32(arr, len(descs), B, kernels._ptr(ws), nbytes, L.stream()), 'inception_conv')
    return [it[3] for it in items]


def pool(x, mode, stride, pad, y=None, y_coff=0):
    """3 x 3 pool: mode 'max' or 'avg' (in-bounds taps only, count_include_pad=False); into y[:, y_coff:y_coff+C] when given."""
    L = kernels._Launch()
    x = L.req(x, 'x')
    B, C, H, W = x.shape
    OH, OW = out_size(H, 3, stride, pad), out_size(W, 3, stride, pad)
    if y is None:
        y = L.new((B, C, OH, OW))
    L.view(y, 'y')
    if tuple(y.shape[2:]) != (OH, OW) or y.shape[0] != B or not y.is_contiguous() or y.dtype != torch.float32:
        raise ShgError(f'inception: pool output {tuple(y.shape)} does not fit input {tuple(x.shape)}')
    with L:
        check(_lib.get_lib().shg_inception_pool_f32(kernels._ptr(x), kernels._ptr(y), B, C, H, W, {'max': 0, 'avg': 1}[mode], stride, pad,
                                                    y.shape[1], y_coff, L.stream()), 'inception_pool')
    return y


def global_mean(x):
    L = kernels._Launch()
    x = L.req(x, 'x')
    B, C = x.shape[:2]
    y = L.new((B, C))
    with L:
        check(_lib.get_lib().shg_inception_mean_f32(kernels._ptr(x), kernels._ptr(y), B, C, x[0, 0].numel(), L.stream()), 'inception_mean')
    return y


def head_probs(feats, w, bias=None):
    """softmax(feats [B, D] @ w [C, D].T (+ bias [C])) -> [B, C] float32 in one launch (csrc/inception.hip: one workgroup per image)."""
    L = kernels._Launch()
    feats, w, bias = L.req(feats, 'feats'), L.req(w, 'head weight'), L.req(bias, 'head bias')
    if feats.ndim != 2 or w.ndim != 2 or w.shape[1] != feats.shape[1] or (bias is not None and tuple(bias.shape) != (w.shape[0],)):
        raise ShgError(f'inception: head: feats [B, D], weight [C, D], bias [C] (got {tuple(feats.shape)}, {tuple(w.shape)})')
    probs = L.new((feats.shape[0], w.shape[0]))
    with L:
        check(_lib.get_lib().shg_inception_head_f32(kernels._ptr(feats), kernels._ptr(w), kernels._ptr(bias), kernels._ptr(probs), feats.shape[0],
                                                    w.shape[0], feats.shape[1], L.stream()), 'inception_head')
    return probs


_LUTS = {}


def value_table(device, input_range):
    """float32 value of every uint8 code as the detector sees it: the byte itself ('0_255', the composite), or the decoded pixel's
    ``u8_value_table`` value mapped by ``*127.5 + 127.5`` in float32 ('pm1', a loader's uint8 reals)."""
    key = (str(device), input_range)
    if key not in _LUTS:
        if input_range == '0_255':
            _LUTS[key] = torch.arange(256, dtype=torch.float32, device=device)
        else:
            _LUTS[key] = kernels.u8_value_table(device) * 127.5 + 127.5
    return _LUTS[key]


def frontend(images, input_range='0_255'):
    """images [B,3,H,W] uint8 or float32 -> [B,3,299,299] float32 = (resize(v) - 128) / 128 (one launch)."""
    if input_range not in ('0_255', 'pm1'):
        raise ShgError(f"inception: input_range must be '0_255' or 'pm1' (got {input_range!r})")
    L = kernels._Launch()
    x, lut, scale, bias = kernels._image_operand(L, images, 'images', lambda dev: value_table(dev, input_range),
                                                 (127.5, 127.5) if input_range == 'pm1' else (1.0, 0.0), 'inception')
    B, _, H, W = x.shape
    y = L.new((B, 3, RES, RES))
    with L:
        check(_lib.get_lib().shg_inception_frontend_f32(kernels._ptr(x), kernels._ptr(lut), scale, bias, kernels._ptr(y), B, H, W, L.stream()),
              'inception_frontend')
    return y


class InceptionFeatures:
    """The detector: ``det(images, return_features=True) -> [B, 2048]``.  Every launch goes to the current stream and every activation
    buffer comes from torch's caching allocator on it, so the detector runs on any stream (EvalLoop's side streams) concurrently with
    itself.  ``split_k=False`` keeps every launch plan independent of the batch size (an image's features are then the same bits in any
    batch); the default splits K in launches too small to fill the chip."""

    def __init__(self, ops, device, split_k=True, head=None):
        self.ops, self.device, self.split_k = ops, torch.device(device), split_k
        self.head = head                # (weight [C, 2048], bias [C]) float32 on the device, or None: features only

    @property
    def num_classes(self):
        return None if self.head is None else int(self.head[0].shape[0])

    @classmethod
    def from_state_dict(cls, sd, device='cuda', split_k=True):
        validate_state_dict(sd, head=HEAD_WEIGHT in sd)
        ops = collections.OrderedDict()
        for name, (i, o, k, s, p, _) in LAYERS.items():
            w, b = fold_bn(sd[f'{name}.conv.weight'], *(sd[f'{name}.bn.{k_}'] for k_ in BN_KEYS))
            wp, bp = pack_weight(w.to(torch.float32).to(device), b.to(torch.float32).to(device))
            ops[name] = ConvOp(name, wp, bp, i, o, k, s, p)
        head = None
        if HEAD_WEIGHT in sd:
            head = tuple(torch.as_tensor(sd[k]).detach().to(torch.float32).to(device).contiguous() for k in (HEAD_WEIGHT, HEAD_BIAS))
        return cls(ops, device, split_k, head)

    def __call__(self, images, return_features=True, input_range='0_255', no_output_bias=True, with_probs=False):
        """``return_features=True``: the pooled features [B, 2048].  ``return_features=False``: the classifier's softmax probabilities
        [B, C] float32, without the output bias by default (the reference's Inception Score passes ``no_output_bias=True``,
        inception_score.py:21).  ``with_probs=True``: (features, probabilities) of ONE run of the trunk (EvalLoop with FID / KID and the
        Inception Score on the same images)."""
        if (with_probs or not return_features) and self.head is None:
            raise ShgError(f'inception: the softmax probabilities need the classifier head, and the state_dict had no {HEAD_WEIGHT!r}')
        with torch.no_grad():
            feats = self.forward(frontend(images, input_range))
            if return_features and not with_probs:
                return feats
            probs = self.probs(feats, no_output_bias)
        return (feats, probs) if with_probs else probs

    def probs(self, feats, no_output_bias=True):
        """Pooled features [B, 2048] -> softmax probabilities [B, C] (one launch)."""
        if self.head is None:
            raise ShgError(f'inception: the softmax probabilities need the classifier head, and the state_dict had no {HEAD_WEIGHT!r}')
        return head_probs(feats, self.head[0], None if no_output_bias else self.head[1])

    def _new(self, B, C, H, W):
        return torch.empty((B, C, H, W), dtype=torch.float32, device=self.device)

    def _run(self, *items):
        conv_group([(self.ops[n], x, 0, y, yo) for n, x, y, yo in items], split_k=self.split_k)

    def forward(self, x):
        """x [B,3,299,299] normalised -> [B, 2048]."""
        B = x.shape[0]
        new, run = self._new, self._run
        for name, c, h in (('Conv2d_1a_3x3', 32, 149), ('Conv2d_2a_3x3', 32, 147), ('Conv2d_2b_3x3', 64, 147)):
            y = new(B, c, h, h)
            run((name, x, y, 0))
            x = y
        x = pool(x, 'max', 2, 0)
        for name, c, h in (('Conv2d_3b_1x1', 80, 73), ('Conv2d_4a_3x3', 192, 71)):
            y = new(B, c, h, h)
            run((name, x, y, 0))
            x = y
        x = pool(x, 'max', 2, 0)
        for name, pf in (('Mixed_5b', 32), ('Mixed_5c', 64), ('Mixed_5d', 64)):
            x = self._block_a(name, x, pf)
        x = self._block_b(x)
        for name, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
            x = self._block_c(name, x, c7)
        x = self._block_d(x)
        x = self._block_e('Mixed_7b', x, 'avg')
        x = self._block_e('Mixed_7c', x, 'max')
        return global_mean(x)

    def _block_a(self, n, x, pf):
        B, _, h, w = x.shape
        out, p = self._new(B, 224 + pf, h, w), pool(x, 'avg', 1, 1)
        t5, t3, t3b = self._new(B, 48, h, w), self._new(B, 64, h, w), self._new(B, 96, h, w)
        self._run((f'{n}.branch1x1', x, out, 0), (f'{n}.branch5x5_1', x, t5, 0), (f'{n}.branch3x3dbl_1', x, t3, 0), (f'{n}.branch_pool', p, out, 224))
        self._run((f'{n}.branch5x5_2', t5, out, 64), (f'{n}.branch3x3dbl_2', t3, t3b, 0))
        self._run((f'{n}.branch3x3dbl_3', t3b, out, 128))
        return out

    def _block_b(self, x):
        n, B = 'Mixed_6a', x.shape[0]
        out, t1, t2 = self._new(B, 768, 17, 17), self._new(B, 64, 35, 35), self._new(B, 96, 35, 35)
        self._run((f'{n}.branch3x3', x, out, 0), (f'{n}.branch3x3dbl_1', x, t1, 0))
        pool(x, 'max', 2, 0, y=out, y_coff=480)
        self._run((f'{n}.branch3x3dbl_2', t1, t2, 0))
        self._run((f'{n}.branch3x3dbl_3', t2, out, 384))
        return out

    def _block_c(self, n, x, c7):
        B, _, h, w = x.shape
        out, p = self._new(B, 768, h, w), pool(x, 'avg', 1, 1)
        a1, a2, d1, d2, d3, d4 = (self._new(B, c7, h, w) for _ in range(6))
        self._run((f'{n}.branch1x1', x, out, 0), (f'{n}.branch7x7_1', x, a1, 0), (f'{n}.branch7x7dbl_1', x, d1, 0), (f'{n}.branch_pool', p, out, 576))
        self._run((f'{n}.branch7x7_2', a1, a2, 0), (f'{n}.branch7x7dbl_2', d1, d2, 0))
        self._run((f'{n}.branch7x7_3', a2, out, 192), (f'{n}.branch7x7dbl_3', d2, d3, 0))
        self._run((f'{n}.branch7x7dbl_4', d3, d4, 0))
        self._run((f'{n}.branch7x7dbl_5', d4, out, 384))
        return out

    def _block_d(self, x):
        n, B = 'Mixed_7a', x.shape[0]
        out = self._new(B, 1280, 8, 8)
        a1, b1, b2, b3 = (self._new(B, 192, 17, 17) for _ in range(4))
        self._run((f'{n}.branch3x3_1', x, a1, 0), (f'{n}.branch7x7x3_1', x, b1, 0))
        pool(x, 'max', 2, 0, y=out, y_coff=512)
        self._run((f'{n}.branch3x3_2', a1, out, 0), (f'{n}.branch7x7x3_2', b1, b2, 0))
        self._run((f'{n}.branch7x7x3_3', b2, b3, 0))
        self._run((f'{n}.branch7x7x3_4', b3, out, 320))
        return out

    def _block_e(self, n, x, pool_mode):
        B, _, h, w = x.shape
        out, p = self._new(B, 2048, h, w), pool(x, pool_mode, 1, 1)
        a1, d1, d2 = self._new(B, 384, h, w), self._new(B, 448, h, w), self._new(B, 384, h, w)
        self._run((f'{n}.branch1x1', x, out, 0), (f'{n}.branch3x3_1', x, a1, 0), (f'{n}.branch3x3dbl_1', x, d1, 0), (f'{n}.branch_pool', p, out, 1856))
        self._run((f'{n}.branch3x3_2a', a1, out, 320), (f'{n}.branch3x3_2b', a1, out, 704), (f'{n}.branch3x3dbl_2', d1, d2, 0))
        self._run((f'{n}.branch3x3dbl_3a', d2, out, 1088), (f'{n}.branch3x3dbl_3b', d2, out, 1472))
        return out


def macs_per_image():
    """Multiply-adds of the 94 convolutions for one 299 x 299 image (the pools, the front end and the mean are not counted)."""
    total = 0
    for i, o, (kh, kw), (sh, sw), (ph, pw), h in LAYERS.values():
        oh, ow = out_size(h, kh, sh, ph), out_size(h, kw, sw, pw)
        total += oh * ow * o * i * kh * kw
    return total
