"""Places2 evaluation input on the device: Pillow-exact bicubic resize of decoded uint8 images (``FixResolutionLoader``,
lib/data_factory/ds_places2.py:90-103: ``Image.resize([R, R], BICUBIC)`` of an RGB image, 8 bits per channel).

Pillow's 8-bit resample (``ImagingResample``) is integer arithmetic on coefficient tables computed in double precision:
  * per axis (in -> out): scale = in/out, fs = max(scale, 1), support = 2 fs; output index i has center (i + .5) scale, taps
    [xmin, xmax) with xmin = max(0, (int)(center - support + .5)), xmax = min(in, (int)(center + support + .5)), weights
    bicubic((x - center + .5) / fs) (a = -0.5) normalised by their sequential sum, then fixed point with 22 fractional bits;
  * horizontal pass first (only when w != R), vertical second (only when h != R), each ``(1 << 21 + sum u8 * k) >> 22`` clipped to
    0..255 -- the intermediate is uint8.
The tables are built here (double precision, the taps accumulated in Pillow's order: vectorised over output indices, looped over
taps), cached per (in, out) pair, and uploaded with the batch; the kernels (csrc/pillow_resample.h) only add integers, so the device result
is bit-exact by construction.  An axis that keeps its size gets the one-tap identity table (k = 1 << 22), which is Pillow's skipped
pass in the same arithmetic.  ``resize_reference`` is the same two passes in numpy (CPU tests).

OpenImages (``FixResolutionLoader`` of lib/data_factory/ds_openimages.py:63-81) resizes only images larger than R, to the box
``fit_size`` keeps their aspect ratio in, and pastes the result at the top-left of a zero R x R canvas: ``build_fit_table`` /
``resize_fit_pad_u8`` (one launch, padding included) and the numpy ``fit_reference``.

Training input of Places2, OpenImages and DTD (``AdvInpaintingFormatter`` / ``InpaintingFormatter``, ds_places2.py:183-207,
ds_openimages.py:117-141, ds_texture.py:121-149): ``randcrop_bicubic`` -- the s x s window of torch's float bicubic resample to a drawn
nh x nw, with the texture formatter's flips, straight from the decoded bytes in one launch (csrc/randcrop.hip); ``randcrop_reference``
is the same arithmetic in numpy float32."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check

PRECISION_BITS = 22
LDS_BYTES = 49152                    # csrc/resize.hip RS_LDS_BYTES: the horizontally resampled band of one workgroup
DESC_INTS = 12                       # csrc/resize.hip: per-image descriptor
FIT_DESC_INTS = 14                   # csrc/resize.hip: per-image descriptor of the fit-and-pad launch (+ h', w')
RANDCROP_DESC_INTS = 9               # csrc/randcrop.hip: h, w, byte offset, nh, nw, ch, cw, flip_v, flip_h
_RANDCROP_LUT = {}
_WEIGHT_CACHE = {}
_COEF_CACHE = {}


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def bicubic_taps(n_in, n_out):
    """-> (xmin int64 [out], n int64 [out], w float64 [out, K]): Pillow's tap range and normalised bicubic weights along one axis, in double
    precision before any rounding (n_in != n_out; weights past a row's n taps are 0)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5), n_in).astype(np.int64)
    n = xmax - xmin
    pre = np.zeros((n_out, ksize), np.float64)
    ww = np.zeros(n_out, np.float64)
    for j in range(ksize):                              # sequential sum over taps, as Pillow's loop
        w = np.where(j < n, _bicubic(((j + xmin) - center + 0.5) * ss), 0.0)
        pre[:, j] = w
        ww = ww + w
    pre = np.where(ww[:, None] != 0.0, pre / np.where(ww == 0.0, 1.0, ww)[:, None], pre)
    return xmin, n, pre


def bicubic_weights(n_in, n_out):
    """-> (bounds int32 [out, 2] = (first tap, taps), w float64 [out, K]): Pillow's bicubic taps along one axis in double precision,
    before any rounding (a size that stays gets the one-tap identity: Pillow skips the pass); cached."""
    key = (int(n_in), int(n_out))
    hit = _WEIGHT_CACHE.get(key)
    if hit is not None:
        return hit
    if key[0] < 1 or key[1] < 1:
        raise ValueError(f'bicubic_weights: sizes must be >= 1 (got {key[0]} -> {key[1]})')
    if key[0] == key[1]:
        bounds = np.stack([np.arange(key[1]), np.ones(key[1], np.int64)], axis=1).astype(np.int32)
        w = np.ones((key[1], 1), np.float64)
    else:
        xmin, n, w = bicubic_taps(*key)
        bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    w.setflags(write=False)
    _WEIGHT_CACHE[key] = (bounds, w)
    return bounds, w


def bicubic_coeffs(in_size, out_size):
    """-> (bounds int32 [out, 2] = (xmin, n), k int32 [out, K]) of Pillow's 8-bit bicubic resample along one axis: ``bicubic_weights`` in
    fixed point (the identity's 1.0 becomes 1 << 22, Pillow's skipped pass in the same arithmetic); cached."""
    key = (int(in_size), int(out_size))
    hit = _COEF_CACHE.get(key)
    if hit is not None:
        return hit
    if key[0] < 1 or key[1] < 1:
        raise ValueError(f'bicubic_coeffs: sizes must be >= 1 (got {key[0]} -> {key[1]})')
    bounds, w = bicubic_weights(*key)
    fx = w * float(1 << PRECISION_BITS)
    k = np.where(w < 0, np.trunc(-0.5 + fx), np.trunc(0.5 + fx)).astype(np.int32)
    k.setflags(write=False)
    _COEF_CACHE[key] = (bounds, k)
    return bounds, k


def _pass(src, bounds, k, axis):
    """One resample pass of Pillow's 8-bit arithmetic along ``axis`` of a uint8 array (int64 accumulation; the int32 bound is a test)."""
    src = np.moveaxis(src, axis, 0).astype(np.int64)
    acc = np.full((k.shape[0],) + src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    xmin, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    tail = (slice(None),) + (None,) * (src.ndim - 1)
    for j in range(k.shape[1]):
        idx = np.minimum(xmin + j, src.shape[0] - 1)
        kj = np.where(j < n, k[:, j], 0).astype(np.int64)
        acc += src[idx] * kj[tail]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_reference(img, R, flip=False):
    """Host reference: uint8 HWC RGB -> uint8 [3, R, R] (horizontal pass, uint8 intermediate, vertical pass; then the flip)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    mid = img if w == R else _pass(img, *bicubic_coeffs(w, R), axis=1)
    out = mid if h == R else _pass(mid, *bicubic_coeffs(h, R), axis=0)
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def fit_size(h, w, R):
    """-> (h', w'): the size FixResolutionLoader (ds_openimages.py:68-72) gives an h x w image at resolution R.  Only images with a side
    above R are resized, to ``(R, int(h * R / w))`` (w > h) or ``(int(w * R / h), R)``, in float64 exactly as written there -- not
    ``h * R // w``: at R = 1024 a 1122 x 1122 image gets (h', w') = (1024, 1023), one column short of the canvas.  A box of 0 pixels
    raises the ValueError Pillow's resize raises."""
    h, w, R = int(h), int(w), int(R)
    if w > R or h > R:
        ratio = R / w if w > h else R / h
        w, h = (R, int(h * ratio)) if w > h else (int(w * ratio), R)
        if w <= 0 or h <= 0:
            raise ValueError('height and width must be > 0')
    return h, w


def fit_reference(img, R, flip=False):
    """Host reference of the OpenImages input: uint8 HWC RGB -> uint8 [3, R, R] = the image resized to ``fit_size`` (Pillow's 8-bit
    bicubic, as resize_reference) at the top-left of a zero canvas, the whole canvas mirrored when ``flip``."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    oh, ow = fit_size(h, w, R)
    mid = img if w == ow else _pass(img, *bicubic_coeffs(w, ow), axis=1)
    out = mid if h == oh else _pass(mid, *bicubic_coeffs(h, oh), axis=0)
    canvas = np.zeros((R, R, 3), np.uint8)
    canvas[:oh, :ow] = out
    if flip:
        canvas = canvas[:, ::-1]
    return np.ascontiguousarray(canvas.transpose(2, 0, 1))


def _tiling(h, oh, R):
    """(band rows TB, column chunk CW, LDS bytes) of one image of h rows resampled to oh <= R box rows on an R-row canvas (oh = R: the
    plain resize): the tallest band (fewest source rows resampled twice by neighbouring bands) whose source rows, resampled to a chunk
    of at most 128 columns, fit the workgroup's LDS (3 planes x rows x chunk, uint8).  The bands cover the canvas, the LDS holds the
    source rows of the box part of a band."""
    bounds, _ = bicubic_coeffs(h, oh)
    lo, hi = bounds[:, 0].astype(np.int64), (bounds[:, 0] + bounds[:, 1]).astype(np.int64)
    for tb in (16, 8, 4, 2, 1):
        tb = min(tb, R)
        starts = np.arange(0, oh, tb)
        span = int((hi[np.minimum(starts + tb, oh) - 1] - lo[starts]).max())
        for cw in (min(R, 128), 64, 32, 16):
            lds = 3 * span * ((cw + 3) // 4 * 4)
            if cw <= R and lds <= LDS_BYTES:
                return tb, cw, lds
    raise ValueError(f'resize: a {h}-row image is too tall to resample to {oh} rows in one workgroup band')


class _Table:
    """The int32 table of one launch while it is assembled: ``desc``, B descriptor rows of ``ints`` ints (int64 until ``finish``), then
    each distinct per-axis (bounds, payload) pair once, with the launch's grid and LDS maxima over the images."""

    def __init__(self, B, ints):
        self.desc = np.zeros((B, ints), np.int64)
        self.parts, self.placed, self.pos = [], {}, B * ints
        self.chunks = self.bands = self.lds_bytes = 1

    def place(self, key, bounds, payload):
        """Append bounds [n, 2] and payload [n, K] (int32) once per ``key`` -> (bounds offset, payload offset, K)."""
        if key not in self.placed:
            self.placed[key] = (self.pos, self.pos + bounds.size, payload.shape[1])
            self.parts.extend([bounds.reshape(-1), payload.reshape(-1)])
            self.pos += bounds.size + payload.size
        return self.placed[key]

    def tile(self, chunks, bands, lds):
        self.chunks, self.bands, self.lds_bytes = max(self.chunks, chunks), max(self.bands, bands), max(self.lds_bytes, lds)

    def finish(self, what, min_lds):
        """-> (int32 table, chunks, bands, LDS bytes)."""
        if self.pos >= 2 ** 31:
            raise ValueError(f'{what}: coefficient table too large')
        table = np.concatenate([self.desc.reshape(-1).astype(np.int32)] + [p.astype(np.int32) for p in self.parts])
        return table, self.chunks, self.bands, max(self.lds_bytes, min_lds)


def build_fit_table(shapes, R, flip=None):
    """Host side of one fit-and-pad launch: shapes int [B, 3] = (h, w, byte offset) -> (int32 table, chunks, bands, LDS bytes).
    table = B descriptors of FIT_DESC_INTS ints (build_table's 12, then the box h', w' of ``fit_size``), then each distinct (in, out)
    pair's bounds and coefficients once (an image that keeps its size on an axis gets the identity table of that size)."""
    shapes = np.asarray(shapes, np.int64).reshape(-1, 3)
    B = shapes.shape[0]
    R = int(R)
    flip = np.zeros(B, np.int64) if flip is None else np.asarray(flip).astype(np.int64).reshape(B)
    t = _Table(B, FIT_DESC_INTS)
    for i, (h, w, off) in enumerate(shapes):
        if h < 1 or w < 1 or off < 0:
            raise ValueError(f'resize: image {i} has shape {h}x{w} at offset {off}')
        oh, ow = fit_size(h, w, R)
        tb, cw, lds = _tiling(int(h), oh, R)
        t.desc[i] = ((h, w, off, flip[i] != 0) + t.place((int(w), ow), *bicubic_coeffs(w, ow)) + t.place((int(h), oh), *bicubic_coeffs(h, oh))
                     + (tb, cw, oh, ow))
        t.tile(-(-R // cw), -(-R // tb), lds)
    return t.finish('resize', 12)


def build_table(shapes, R, flip=None):
    """Host side of one launch: shapes int [B, 3] = (h, w, byte offset of the HWC image) -> (int32 table, chunks, bands, LDS bytes).
    table = B descriptors of DESC_INTS ints (h, w, offset, flip, horizontal bounds / coefficients / width, vertical bounds /
    coefficients / width, band rows, column chunk), then each distinct (in, R) pair's bounds and coefficients once."""
    shapes = np.asarray(shapes, np.int64).reshape(-1, 3)
    B = shapes.shape[0]
    flip = np.zeros(B, np.int64) if flip is None else np.asarray(flip).astype(np.int64).reshape(B)
    t = _Table(B, DESC_INTS)
    for i, (h, w, off) in enumerate(shapes):
        if h < 1 or w < 1 or off < 0:
            raise ValueError(f'resize: image {i} has shape {h}x{w} at offset {off}')
        tb, cw, lds = _tiling(int(h), R, R)
        t.desc[i] = (h, w, off, flip[i] != 0) + t.place(int(w), *bicubic_coeffs(w, R)) + t.place(int(h), *bicubic_coeffs(h, R)) + (tb, cw)
        t.tile(-(-R // cw), -(-R // tb), lds)
    return t.finish('resize', 12)


def _upload(host, dev):
    """numpy array -> tensor on ``dev`` through pinned memory; the copy is asynchronous on the current stream."""
    return torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)


def _launch_resize(name, build, packed, shapes, R, flip, stream):
    """The body of ``resize_bicubic_u8`` / ``resize_fit_pad_u8``: ``build`` makes the launch's table, ``shg_<name>`` consumes it."""
    if not (isinstance(packed, torch.Tensor) and packed.is_cuda and packed.dtype == torch.uint8):
        raise _lib.ShgError(f'{name}: packed must be a uint8 HIP tensor: libshgan_hip has no CPU path')
    packed = packed.contiguous().view(-1)
    shapes = shapes.numpy() if isinstance(shapes, torch.Tensor) else shapes
    flip = flip.numpy() if isinstance(flip, torch.Tensor) else flip
    R = int(R)
    table, chunks, bands, lds_bytes = build(shapes, R, flip)
    B = np.asarray(shapes).reshape(-1, 3).shape[0]
    dev = packed.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        tab = _upload(table, dev)
        out = torch.empty((B, 3, R, R), dtype=torch.uint8, device=dev)
        check(getattr(_lib.get_lib(), 'shg_' + name)(ctypes.c_void_p(packed.data_ptr()), packed.numel(), ctypes.c_void_p(tab.data_ptr()),
                                                     tab.numel(), ctypes.c_void_p(out.data_ptr()), B, R, chunks, bands, lds_bytes,
                                                     ctypes.c_void_p(st.cuda_stream)), name)
    return out


def resize_bicubic_u8(packed, shapes, R, flip=None, stream=None):
    """packed: uint8 HIP tensor holding B HWC RGB images back to back; shapes: host int [B, 3] = (h, w, byte offset) (numpy or a CPU
    tensor); flip: host [B] flags (horizontal flip of the resized image) or None -> uint8 [B, 3, R, R] on packed's device, computed on
    ``stream`` (default: the current stream).  The coefficient table travels with the launch (pinned, asynchronous)."""
    return _launch_resize('resize_bicubic_u8', build_table, packed, shapes, R, flip, stream)


def resize_fit_pad_u8(packed, shapes, R, flip=None, stream=None):
    """The OpenImages input: packed / shapes / flip / stream as resize_bicubic_u8 -> uint8 [B, 3, R, R], image i resized to
    ``fit_size(h, w, R)`` at the top-left of a zero canvas (the whole canvas mirrored when flip[i]).  One launch writes every byte."""
    return _launch_resize('resize_fit_pad_u8', build_fit_table, packed, shapes, R, flip, stream)


def pack_images(images):
    """list of uint8 HWC RGB arrays -> (packed uint8 tensor [sum h w 3], shapes int32 [B, 3] = (h, w, offset))."""
    shapes = np.zeros((len(images), 3), np.int64)
    off = 0
    for i, im in enumerate(images):
        h, w = im.shape[:2]
        if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
            raise ValueError('pack_images: images must be uint8 HWC RGB')
        shapes[i] = (h, w, off)
        off += h * w * 3
    if off >= 2 ** 31:
        raise ValueError('pack_images: a batch holds at most 2 GiB of pixels')
    packed = torch.empty(off, dtype=torch.uint8)
    buf = packed.numpy()
    for im, (h, w, o) in zip(images, shapes):
        buf[o:o + h * w * 3] = np.ascontiguousarray(im).reshape(-1)
    return packed, torch.from_numpy(shapes.astype(np.int32))


# ------------------------------------------------------------------------------------------------
# random scale, random crop: the training formatter of Places2 / OpenImages / DTD
# ------------------------------------------------------------------------------------------------

def randcrop_value_table():
    """float32 [256]: the value the reference's formatter gives a byte -- ToTensor (``byte / 255``), then ``(v - 0.5) * 2``, each in
    float32 (ds_places2.py:196-197)."""
    return (np.arange(256, dtype=np.float32) / np.float32(255) - np.float32(0.5)) * np.float32(2)


def _randcrop_lut(device):
    key = str(device)
    if key not in _RANDCROP_LUT:
        _RANDCROP_LUT[key] = torch.from_numpy(randcrop_value_table()).to(device)
    return _RANDCROP_LUT[key]


def randcrop_desc(shapes, params):
    """shapes int [B,3] = (h, w, byte offset), params int [B,6] = (nh, nw, ch, cw, flip_v, flip_h) -> the launch's int32 [B,9]
    descriptor rows (h, w, offset, nh, nw, ch, cw, flip_v, flip_h)."""
    shapes = np.asarray(shapes.numpy() if isinstance(shapes, torch.Tensor) else shapes, np.int64).reshape(-1, 3)
    params = np.asarray(params.numpy() if isinstance(params, torch.Tensor) else params, np.int64).reshape(-1, 6)
    if shapes.shape[0] != params.shape[0]:
        raise ValueError(f'randcrop: {shapes.shape[0]} images but {params.shape[0]} parameter rows')
    desc = np.concatenate([shapes, params], axis=1)
    if desc.size and (np.abs(desc).max() >= 2 ** 31):
        raise ValueError('randcrop: descriptor values must fit int32')
    return np.ascontiguousarray(desc.astype(np.int32))


def _cubic_axis(n_in, n_out, dst):
    """torch's float32 source coordinate and cubic weights (A = -0.75) of the output indices ``dst`` along one axis ->
    (first tap index i0 - 1, unclamped, int64 [n]; weights float32 [n, 4]); every step rounded to float32, in the kernel's order."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    src = scale * (np.asarray(dst).astype(f) + f(0.5)) - f(0.5)
    fl = np.floor(src)
    t = src - fl
    A = f(-0.75)
    x0, x1, x2, x3 = t + f(1), t, f(1) - t, f(2) - t

    def inner(x):
        return ((A + f(2)) * x - (A + f(3))) * x * x + f(1)

    def outer(x):
        return ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A

    w = np.stack([outer(x0), inner(x1), inner(x2), outer(x3)], axis=1)
    assert w.dtype == f
    return fl.astype(np.int64) - 1, w


def _fma32(a, b, c):
    """float32 fma: the product is exact in float64; the sum is rounded to float64 and then to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def randcrop_reference(img, s, params):
    """Host reference of one image: uint8 HWC RGB, params = (nh, nw, ch, cw, flip_v, flip_h) -> float32 [3, s, s], the kernel's
    arithmetic in numpy float32 (float32 coordinates and weights; per tap row the sum along x, then the four row sums along y, each
    ``w0 * v0`` followed by three fused multiply-adds)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    nh, nw, ch, cw, fv, fh = (int(v) for v in params)
    s = int(s)
    if s < 1 or nh < s or nw < s or ch < 0 or cw < 0 or ch + s > nh or cw + s > nw or h < 1 or w < 1:
        raise ValueError(f'randcrop_reference: window [{ch}:{ch}+{s}, {cw}:{cw}+{s}] of {nh}x{nw} from a {h}x{w} image')
    v = randcrop_value_table()[img]                                               # [h, w, 3]
    ix, wx = _cubic_axis(w, nw, cw + np.arange(s))
    iy, wy = _cubic_axis(h, nh, ch + np.arange(s))
    cols = np.clip(ix[:, None] + np.arange(4), 0, w - 1)                          # [s, 4]
    rows = np.clip(iy[:, None] + np.arange(4), 0, h - 1)
    out = None
    for jy in range(4):
        r = v[rows[:, jy]]                                                        # [s, w, 3]
        hsum = wx[None, :, 0, None] * r[:, cols[:, 0]]
        for jx in range(1, 4):
            hsum = _fma32(np.broadcast_to(wx[None, :, jx, None], hsum.shape), r[:, cols[:, jx]], hsum)
        wj = np.broadcast_to(wy[:, jy, None, None], hsum.shape)
        out = wj * hsum if out is None else _fma32(wj, hsum, out)
    assert out.dtype == np.float32
    if fv:
        out = out[::-1]
    if fh:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def randcrop_bicubic(src, desc_or_shapes, s, params=None, stream=None):
    """The window launch.  Two source forms:
      * ragged: ``src`` uint8 HIP tensor of packed HWC images (``pack_images`` / ``RaggedU8Batch.data``), ``desc_or_shapes`` the host
        int [B,3] shapes (h, w, byte offset);
      * planar: ``src`` uint8 HIP tensor [B,3,H,W] (what ``resize_bicubic_u8`` / ``resize_fit_pad_u8`` return), ``desc_or_shapes`` None.
    ``params`` host int [B,6] = (nh, nw, ch, cw, flip_v, flip_h).  Alternatively ``desc_or_shapes`` is the full int [B,9] descriptor
    (``randcrop_desc``) and ``params`` None.  -> float32 [B,3,s,s] in [-1, 1] (up to the cubic's overshoot) on src's device, computed
    on ``stream`` (default: the current stream); the descriptor travels with the launch (pinned, asynchronous)."""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
        raise _lib.ShgError('randcrop_bicubic: src must be a uint8 HIP tensor: libshgan_hip has no CPU path')
    planar = src.ndim == 4
    if planar:
        if src.shape[1] != 3:
            raise _lib.ShgError(f'randcrop_bicubic: a planar source is [B,3,H,W] (got {tuple(src.shape)})')
        src = src.contiguous()
        B, _, H, W = src.shape
        if desc_or_shapes is None:
            desc_or_shapes = np.stack([np.full(B, H), np.full(B, W), np.arange(B) * (3 * H * W)], axis=1)
    else:
        src = src.contiguous().view(-1)
    d = np.asarray(desc_or_shapes.numpy() if isinstance(desc_or_shapes, torch.Tensor) else desc_or_shapes)
    if d.ndim == 2 and d.shape[1] == RANDCROP_DESC_INTS and params is None:
        desc = np.ascontiguousarray(d.astype(np.int32))
    elif params is None:
        raise _lib.ShgError('randcrop_bicubic: params (nh, nw, ch, cw, flip_v, flip_h) are required with shapes')
    else:
        desc = randcrop_desc(d, params)
    B, s = desc.shape[0], int(s)
    dev = src.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    fn = _lib.get_lib().shg_randcrop_bicubic_planar_f32 if planar else _lib.get_lib().shg_randcrop_bicubic_ragged_f32
    with torch.cuda.device(dev), torch.cuda.stream(st):
        lut = _randcrop_lut(dev)
        dd = _upload(desc, dev)
        out = torch.empty((B, 3, max(s, 0), max(s, 0)), dtype=torch.float32, device=dev)
        check(fn(ctypes.c_void_p(src.data_ptr()), src.numel(), desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                 ctypes.c_void_p(dd.data_ptr()), ctypes.c_void_p(lut.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, s,
                 ctypes.c_void_p(st.cuda_stream)), 'randcrop_bicubic')
    return out
