"""Inpaint photographs of any size: choose the window the network sees, gather it at the network's resolution, paste the result back into
the original bytes without a seam (csrc/inpaint.hip).

Conventions: masks are the project's (1 / non-zero = known, 0 = hole); images are decoded uint8 HWC RGB packed back to back
(``resize.pack_images``), masks uint8 HW packed the same way (``pack_masks``).  ``shapes`` is the host int [B, 3] = (h, w, image byte offset)
of ``pack_images`` -- the masks then lie back to back in the same order -- or [B, 4] with the mask's byte offset in the last column;
``windows`` is a host int [B, 4] = (y0, x0, ch, cw), every window inside its image.

  * ``plan_window``: the window rule (host, integers).
  * ``gather_windows``: one launch, ragged batch -> (real uint8 [B,3,R,R], mask float32 [B,1,R,R]) for ``eval_harness.assemble_input``.
    The image bytes are Pillow's ``crop(box).resize((R, R), BICUBIC)``; a low-resolution pixel is known iff its whole native footprint is.
  * ``paste_back``: one launch over the windows of K copies of the originals: feather weight A from the native mask (Chebyshev distance,
    an integer 0 .. feather + 1), float32 bicubic resample of the generator's output to the window, scale, blend, truncation.
  * ``Inpainter``: plan, pack, gather -> assemble -> G -> paste, one device-to-host copy per chunk.

The arithmetic is stated with the kernels (csrc/inpaint.hip) and restated in numpy by tests/inpaint_f64.py."""
import ctypes
import math

import numpy as np
import torch

from . import _lib, eval_harness, kernels, resize
from ._lib import check

LDS_BYTES = 49152                    # csrc/inpaint.hip IP_LDS_BYTES
DESC_INTS = 16                       # csrc/inpaint.hip IP_DESC
MAX_FEATHER = 32                     # csrc/inpaint.hip IP_MAX_FEATHER
_WEIGHT_CACHE = {}


def plan_window(mask, R, context=0.5, feather=8):
    """mask: uint8 / bool HW (0 = hole) -> (y0, x0, ch, cw), or None when the mask has no hole.  With the hole's bounding box bh x bw:
    s = max(R, ceil((1 + 2 context) max(bh, bw)), max(bh, bw) + 2 (feather + 2)), ch = min(s, H), cw = min(s, W); the window is centred
    on the box and shifted to lie inside the image.  It is square whenever the image allows; otherwise it is rectangular and is resized
    anisotropically, as the Places2 loader resizes whole images."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f'plan_window: the mask must be HW (got shape {m.shape})')
    H, W = m.shape
    hole = m == 0
    rows, cols = np.flatnonzero(hole.any(axis=1)), np.flatnonzero(hole.any(axis=0))
    if rows.size == 0:
        return None
    ya, yb, xa, xb = int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1
    side = max(yb - ya, xb - xa)
    s = max(int(R), int(math.ceil((1.0 + 2.0 * float(context)) * side)), side + 2 * (int(feather) + 2))
    ch, cw = min(s, H), min(s, W)
    y0 = min(max((ya + yb - ch) // 2, 0), H - ch)
    x0 = min(max((xa + xb - cw) // 2, 0), W - cw)
    return y0, x0, ch, cw


def pack_masks(masks):
    """list of uint8 / bool HW masks -> (packed uint8 tensor [sum h w], byte offsets int64 [B])."""
    offs = np.zeros(len(masks), np.int64)
    off = 0
    for i, m in enumerate(masks):
        if np.ndim(m) != 2:
            raise ValueError('pack_masks: masks must be HW')
        offs[i] = off
        off += int(np.shape(m)[0]) * int(np.shape(m)[1])
    if off >= 2 ** 31:
        raise ValueError('pack_masks: a batch holds at most 2 GiB of pixels')
    buf = np.zeros(off, np.uint8)
    for m, o in zip(masks, offs):
        m = np.asarray(m)
        buf[o:o + m.size] = (m != 0).reshape(-1)
    return torch.from_numpy(buf), offs


def bicubic_weights(n_in, n_out):
    """-> (bounds int32 [out, 2] = (first tap, taps), w float64 [out, K]): Pillow's bicubic taps along one axis exactly as
    ``resize.bicubic_coeffs`` has them before its fixed-point rounding (a size that stays gets the one-tap identity); cached."""
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
        xmin, n, w = resize.bicubic_taps(*key)
        bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    w.setflags(write=False)
    _WEIGHT_CACHE[key] = (bounds, w)
    return bounds, w


def _host(a):
    return np.asarray(a.numpy() if isinstance(a, torch.Tensor) else a)


def _geometry(shapes, windows, what):
    """-> int64 [B, 8] = (h, w, image offset, mask offset, y0, x0, ch, cw), checked."""
    shapes = _host(shapes).astype(np.int64)
    shapes = shapes.reshape(-1, 4 if shapes.ndim == 2 and shapes.shape[1] == 4 else 3)
    windows = _host(windows).astype(np.int64).reshape(-1, 4)
    if shapes.shape[0] != windows.shape[0] or shapes.shape[0] < 1:
        raise ValueError(f'{what}: {shapes.shape[0]} images but {windows.shape[0]} windows (at least one of each)')
    if shapes.shape[1] == 3:
        px = shapes[:, 0] * shapes[:, 1]
        shapes = np.concatenate([shapes, (np.cumsum(px) - px)[:, None]], axis=1)
    geo = np.concatenate([shapes, windows], axis=1)
    for i, (h, w, off, moff, y0, x0, ch, cw) in enumerate(geo):
        if h < 1 or w < 1 or off < 0 or moff < 0:
            raise ValueError(f'{what}: image {i} has shape {h}x{w} at offsets {off} / {moff}')
        if y0 < 0 or x0 < 0 or ch < 1 or cw < 1 or y0 + ch > h or x0 + cw > w:
            raise ValueError(f'{what}: window [{y0}:{y0}+{ch}, {x0}:{x0}+{cw}] of image {i} does not lie inside its {h}x{w} pixels')
    if np.abs(geo).max() >= 2 ** 31:
        raise ValueError(f'{what}: descriptor values must fit int32')
    return geo


def _finish_table(desc, parts, pos, what):
    if pos >= 2 ** 31:
        raise ValueError(f'{what}: coefficient table too large')
    return np.concatenate([desc.reshape(-1).astype(np.int32)] + parts)


def build_gather_table(shapes, windows, R):
    """Host side of a ``gather_windows`` launch -> (int32 table, chunks, bands, LDS bytes): B descriptors of DESC_INTS ints (h, w, image
    offset, mask offset, y0, x0, ch, cw, horizontal bounds / coefficients / width, vertical bounds / coefficients / width, band rows,
    column chunk), then each distinct (in, R) pair's fixed-point table of ``resize.bicubic_coeffs`` once."""
    geo = _geometry(shapes, windows, 'gather_windows')
    R = int(R)
    if R < 1:
        raise ValueError(f'gather_windows: R must be >= 1 (got {R})')
    B = geo.shape[0]
    desc = np.zeros((B, DESC_INTS), np.int64)
    parts, placed, pos = [], {}, B * DESC_INTS

    def place(n_in):
        nonlocal pos
        if n_in not in placed:
            bounds, k = resize.bicubic_coeffs(n_in, R)
            placed[n_in] = (pos, pos + bounds.size, k.shape[1])
            parts.extend([bounds.reshape(-1).astype(np.int32), k.reshape(-1).astype(np.int32)])
            pos += bounds.size + k.size
        return placed[n_in]

    chunks = bands = lds_bytes = 1
    for i, g in enumerate(geo):
        ch, cw = int(g[6]), int(g[7])
        try:
            tb, cc, lds = resize._tiling(ch, R)
        except ValueError:
            raise ValueError(f'gather_windows: the {ch}-row window of image {i} is too tall to resample to {R} rows in one workgroup band') from None
        desc[i] = tuple(g) + place(cw) + place(ch) + (tb, cc)
        chunks, bands, lds_bytes = max(chunks, -(-R // cc)), max(bands, -(-R // tb)), max(lds_bytes, lds)
    return _finish_table(desc, parts, pos, 'gather_windows'), chunks, bands, max(lds_bytes, 12)


def _align16(n):
    return (n + 15) // 16 * 16


def _paste_tiling(ch, cw, R, feather):
    """(band rows TB, column chunk CW, LDS bytes) of one window: the tallest band, then the widest chunk, whose staging fits the
    workgroup's LDS -- a 16-byte flag and A [TB][CW] bytes beside the larger of (hole flags with their halo + row distances) and (the rows of ``fake`` under
    the band, resampled to the chunk: float [rows][3 CW]); csrc/inpaint.hip computes the same sum."""
    bounds, _ = bicubic_weights(R, ch)
    lo, hi = bounds[:, 0].astype(np.int64), (bounds[:, 0] + bounds[:, 1]).astype(np.int64)
    for tb in (16, 8, 4, 2, 1):
        tb = min(tb, ch)
        starts = np.arange(0, ch, tb)
        span = int((hi[np.minimum(starts + tb, ch) - 1] - lo[starts]).max())
        for cc in (128, 64, 32, 16):
            cc = min(cc, cw)
            th, tw = tb + 2 * feather, cc + 2 * feather
            lds = 16 + _align16(tb * cc) + max(_align16(th * ((tw + 3) // 4 * 4)) + _align16(th * cc), 12 * span * cc)
            if lds <= LDS_BYTES:
                return tb, cc, lds
    return None


def build_paste_table(shapes, windows, R, feather):
    """Host side of a ``paste_back`` launch -> (int32 table, chunks, bands, LDS bytes): descriptors as ``build_gather_table``, then each
    distinct (R, out) pair's bounds (int32) and float32 weights (``bicubic_weights`` rounded once; stored as their bit patterns)."""
    geo = _geometry(shapes, windows, 'paste_back')
    R, feather = int(R), int(feather)
    if R < 1 or not 0 <= feather <= MAX_FEATHER:
        raise ValueError(f'paste_back: R must be >= 1 and feather in 0..{MAX_FEATHER} (got {R}, {feather})')
    B = geo.shape[0]
    desc = np.zeros((B, DESC_INTS), np.int64)
    parts, placed, pos = [], {}, B * DESC_INTS

    def place(n_out):
        nonlocal pos
        if n_out not in placed:
            bounds, w = bicubic_weights(R, n_out)
            placed[n_out] = (pos, pos + bounds.size, w.shape[1])
            parts.extend([bounds.reshape(-1).astype(np.int32), np.ascontiguousarray(w.astype(np.float32)).reshape(-1).view(np.int32)])
            pos += bounds.size + w.size
        return placed[n_out]

    chunks = bands = lds_bytes = 1
    for i, g in enumerate(geo):
        ch, cw = int(g[6]), int(g[7])
        tiling = _paste_tiling(ch, cw, R, feather)
        if tiling is None:
            raise ValueError(f'paste_back: image {i}: {R} rows resampled down to a {ch}-row window do not fit one workgroup band '
                             f'(a window that small is not pasted from a {R} x {R} output)')
        tb, cc, lds = tiling
        desc[i] = tuple(g) + place(cw) + place(ch) + (tb, cc)
        chunks, bands, lds_bytes = max(chunks, -(-cw // cc)), max(bands, -(-ch // tb)), max(lds_bytes, lds)
    if chunks > 65535 or bands > 65535:
        raise ValueError('paste_back: a window has more than 65535 bands or chunks')
    return _finish_table(desc, parts, pos, 'paste_back'), chunks, bands, max(lds_bytes, 32)


def _u8_flat(launch, t, name, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise _lib.ShgError(f'{what}: {name} must be a uint8 HIP tensor: libshgan_hip has no CPU path')
    return launch.req(t, name, dtype=torch.uint8).view(-1)


def _upload(table, dev):
    tab = torch.from_numpy(table)
    return tab.pin_memory().to(dev, non_blocking=True)


def _check_extent(geo, n_img, n_mask, what):
    for i, (h, w, off, moff) in enumerate(geo[:, :4]):
        if off + 3 * h * w > n_img or moff + h * w > n_mask:
            raise _lib.ShgError(f'{what}: image {i} ({h}x{w} at {off} / {moff}) does not lie inside packed ({n_img} bytes) / packed_mask ({n_mask} bytes)')


def gather_windows(packed, packed_mask, shapes, windows, R, stream=None):
    """-> (real uint8 [B,3,R,R], mask float32 [B,1,R,R]) on packed's device, computed on ``stream`` (default: the current stream) in one
    launch.  Image i is Pillow's ``crop(window i).resize((R, R), BICUBIC)`` of the packed image, byte for byte (upscaling axes included);
    mask pixel (i, j) is 1 iff every native pixel of rows [i ch // R, max(ceil((i + 1) ch / R), lo + 1)) x the same columns is known."""
    launch = kernels._Launch()               # (``launch``, not ``L``: the allocation tests cover this function from tests/test_gpu_inpaint.py)
    packed = _u8_flat(launch, packed, 'packed', 'gather_windows')
    packed_mask = _u8_flat(launch, packed_mask, 'packed_mask', 'gather_windows')
    R = int(R)
    geo = _geometry(shapes, windows, 'gather_windows')
    _check_extent(geo, packed.numel(), packed_mask.numel(), 'gather_windows')
    table, chunks, bands, lds_bytes = build_gather_table(geo[:, :4], geo[:, 4:], R)
    B = geo.shape[0]
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    with launch, torch.cuda.stream(st):
        tab = _upload(table, launch.dev)
        real = launch.new((B, 3, R, R), torch.uint8)
        mask = launch.new((B, 1, R, R), torch.float32)
        check(_lib.get_lib().shg_inpaint_gather_u8(kernels._ptr(packed), packed.numel(), kernels._ptr(packed_mask), packed_mask.numel(),
                                                   kernels._ptr(tab), tab.numel(), kernels._ptr(real), kernels._ptr(mask), B, R, chunks, bands,
                                                   lds_bytes, ctypes.c_void_p(st.cuda_stream)), 'gather_windows')
    return real, mask


def paste_back(packed, packed_mask, shapes, windows, fake, k=1, feather=8, out=None, alpha_out=None, stream=None):
    """fake: float32 [B k, 3, R, R], the raw generator output, row n k + j = sample j of image n (``sample_many``'s layout) -> out uint8
    [k, len(packed)]: sample j of image n at image n's offset in row j.  ``out`` (made when None) starts as k copies of ``packed`` (one
    ``copy_``); the launch covers the windows only and stores nothing where the feather weight is 0, so every byte away from the hole is
    the original's.  ``feather`` in 0..32 (0: the hard composite).  ``alpha_out``: an optional uint8 tensor in packed-mask layout that
    receives the weight A (0 outside the windows).  One launch on ``stream`` (default: the current stream), no synchronisation."""
    launch = kernels._Launch()
    packed = _u8_flat(launch, packed, 'packed', 'paste_back')
    packed_mask = _u8_flat(launch, packed_mask, 'packed_mask', 'paste_back')
    k, feather = int(k), int(feather)
    if k < 1 or not 0 <= feather <= MAX_FEATHER:
        raise _lib.ShgError(f'paste_back: k must be >= 1 and feather in 0..{MAX_FEATHER} (got {k}, {feather})')
    geo = _geometry(shapes, windows, 'paste_back')
    B = geo.shape[0]
    if not isinstance(fake, torch.Tensor) or fake.ndim != 4 or fake.shape[0] != B * k or fake.shape[1] != 3 or fake.shape[2] != fake.shape[3]:
        raise _lib.ShgError(f'paste_back: fake must be float32 [{B * k}, 3, R, R] (got {tuple(getattr(fake, "shape", ()))})')
    fake = launch.req(fake, 'fake')
    R = fake.shape[2]
    _check_extent(geo, packed.numel(), packed_mask.numel(), 'paste_back')
    table, chunks, bands, lds_bytes = build_paste_table(geo[:, :4], geo[:, 4:], R, feather)
    n = packed.numel()
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (k, n) and out.is_contiguous()):
            raise _lib.ShgError(f'paste_back: out must be a contiguous uint8 HIP tensor [{k}, {n}]')
        launch._own(out, 'out')
    if alpha_out is not None:
        if not (isinstance(alpha_out, torch.Tensor) and alpha_out.is_cuda and alpha_out.dtype == torch.uint8 and alpha_out.is_contiguous()
                and alpha_out.numel() == packed_mask.numel()):
            raise _lib.ShgError(f'paste_back: alpha_out must be a contiguous uint8 HIP tensor of {packed_mask.numel()} bytes')
        launch._own(alpha_out, 'alpha_out')
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    with launch, torch.cuda.stream(st):
        tab = _upload(table, launch.dev)
        if out is None:
            out = launch.new((k, n), torch.uint8)
        out.copy_(packed.view(1, n).expand(k, n))
        if alpha_out is not None:
            alpha_out.zero_()
        check(_lib.get_lib().shg_inpaint_paste_u8(kernels._ptr(out), n, kernels._ptr(packed_mask), packed_mask.numel(), kernels._ptr(tab), tab.numel(),
                                                  kernels._ptr(fake), kernels._ptr(alpha_out), B, k, R, feather, chunks, bands, lds_bytes,
                                                  ctypes.c_void_p(st.cuda_stream)), 'paste_back')
    return out


class Inpainter:
    """``Inpainter(G, resolution, device)(images, masks)`` -> the images with their holes filled.

    images: uint8 [h, w, 3] arrays of any sizes; masks: [h, w] arrays, 0 = hole.  Per image the window of ``plan_window`` is gathered at
    ``resolution``, assembled (``eval_harness.assemble_input``), run through ``G`` (``G.sample_many`` when ``samples > 1``) and pasted
    back with a feather of ``feather`` native pixels.  The result is a list in the order of the inputs: one [h, w, 3] uint8 array per
    image, or [samples, h, w, 3] when ``samples > 1``.  An image without a hole comes back as a copy and never reaches the device.  Images
    are processed in chunks of ``batch``; a chunk is one upload, the launches (no host synchronisation between them) and one
    device-to-host copy.  ``gather_fn`` / ``paste_fn`` (the signatures of ``gather_windows`` / ``paste_back``) and ``G`` can be replaced,
    so the flow also runs on the host with reference functions and a stand-in generator."""

    def __init__(self, G, resolution, device, context=0.5, feather=8, noise_mode='const', batch=16, gather_fn=None, paste_fn=None):
        if int(batch) < 1 or not 0 <= int(feather) <= MAX_FEATHER or int(resolution) < 1:
            raise ValueError(f'Inpainter: batch >= 1, resolution >= 1 and feather in 0..{MAX_FEATHER} are required')
        self.G, self.resolution, self.device = G, int(resolution), torch.device(device)
        self.context, self.feather, self.noise_mode, self.batch = float(context), int(feather), noise_mode, int(batch)
        self.gather_fn = gather_windows if gather_fn is None else gather_fn
        self.paste_fn = paste_back if paste_fn is None else paste_fn

    def _latents(self, n, samples, seed, first):
        """z of images first .. first + n - 1 of the call: image i, sample j draws from the generator seeded ``seed + i`` (so a result does
        not depend on the chunking)."""
        z_dim = int(getattr(self.G, 'z_dim', 512))
        z = np.stack([np.random.RandomState(int(seed) + first + i).standard_normal((samples, z_dim)).astype(np.float32) for i in range(n)])
        return torch.from_numpy(z)

    def _chunk(self, images, masks, windows, z, samples):
        packed, shapes = resize.pack_images(images)
        packed_mask, moffs = pack_masks(masks)
        shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
        windows = np.asarray(windows, np.int64)
        dev = self.device
        if dev.type == 'cuda':
            packed, packed_mask = packed.pin_memory().to(dev, non_blocking=True), packed_mask.pin_memory().to(dev, non_blocking=True)
        z = z.to(dev)
        with torch.no_grad():
            real, m = self.gather_fn(packed, packed_mask, shapes, windows, self.resolution)
            x = eval_harness.assemble_input(real, m)
            if samples > 1:
                fake = self.G.sample_many(x, z, None, noise_mode=self.noise_mode)
                fake = fake.reshape((-1,) + tuple(fake.shape[2:]))
            else:
                fake = self.G(x=x, z=z[:, 0], c=z[:, 0, :0], noise_mode=self.noise_mode)
            out = self.paste_fn(packed, packed_mask, shapes, windows, fake.float(), k=samples, feather=self.feather)
        host = out.cpu().numpy()                                                    # the chunk's one device-to-host copy (it synchronises)
        res = []
        for (h, w, off) in shapes[:, :3]:
            a = host[:, off:off + 3 * h * w].reshape(samples, h, w, 3)
            res.append(a.copy() if samples > 1 else a[0].copy())
        return res

    def __call__(self, images, masks, z=None, samples=1, seed=0):
        samples = int(samples)
        if len(images) != len(masks) or samples < 1:
            raise ValueError(f'Inpainter: {len(images)} images, {len(masks)} masks, samples = {samples}')
        if getattr(self.G, 'c_dim', 0):
            raise ValueError('Inpainter: a conditional generator (c_dim > 0) is not served')
        images = [np.asarray(im) for im in images]
        for i, (im, mk) in enumerate(zip(images, masks)):
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or tuple(np.shape(mk)) != im.shape[:2]:
                raise ValueError(f'Inpainter: image {i} must be uint8 [h, w, 3] with a mask [h, w]')
        windows = [plan_window(mk, self.resolution, self.context, self.feather) for mk in masks]
        todo = [i for i, wnd in enumerate(windows) if wnd is not None]
        if z is not None:
            z = torch.as_tensor(z, dtype=torch.float32).cpu()
            z = z[:, None] if z.ndim == 2 else z
            if z.ndim != 3 or z.shape[0] != len(images) or z.shape[1] != samples:
                raise ValueError(f'Inpainter: z must be [{len(images)}, z_dim] or [{len(images)}, {samples}, z_dim] (got {tuple(z.shape)})')
        result = [None] * len(images)
        for i, wnd in enumerate(windows):
            if wnd is None:
                result[i] = np.broadcast_to(images[i], (samples,) + images[i].shape).copy() if samples > 1 else images[i].copy()
        for s in range(0, len(todo), self.batch):
            ids = todo[s:s + self.batch]
            zc = torch.cat([self._latents(1, samples, seed, i) for i in ids]) if z is None else z[ids]
            for i, r in zip(ids, self._chunk([images[i] for i in ids], [masks[i] for i in ids], [windows[i] for i in ids], zc, samples)):
                result[i] = r
        return result
