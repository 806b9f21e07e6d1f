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
  * ``paste_back_membrane``: the gradient-domain paste-back (csrc/membrane.hip): ``membrane_setup`` -> ``membrane_solve`` ->
    ``membrane_paste``.  The generated window keeps its gradients and takes its level from the photograph at the rim of the blended
    region Omega = {A > 0}: a membrane c with c = orig - g on the window pixels with A = 0 (0 outside the window) and a vanishing
    5-point Laplacian in Omega is added to g before the feathered blend.  The solve is a multigrid V-cycle on the device with a
    certified stop rule; INTEGRATION section S states the problem, the states and the workspace.
  * ``label_holes`` -> ``fetch_components`` -> ``plan_windows`` -> ``owner_plane``: one window per GROUP of holes (csrc/hole_label.hip):
    the 8-connected components of the mask dilated by feather + 1 are labelled on the device, every group gets ``plan_window``'s window
    for its own hole box and a key, and the paste-backs take the owner plane and the windows' keys (``owner=, keys=``) to blend every
    window's own holes only.  INTEGRATION section T holds the definitions.
  * ``Inpainter``: plan, pack, gather -> assemble -> G -> paste, one device-to-host copy per chunk; ``blend='membrane'`` selects the
    gradient-domain paste-back, ``windows='per_hole'`` one window per group of holes.

The arithmetic is stated with the kernels (csrc/inpaint.hip) and restated in numpy by tests/inpaint_f64.py."""
import ctypes
import math

import numpy as np
import torch

from . import _lib, eval_harness, kernels, resize
from ._lib import check
from .resize import _upload, bicubic_weights

LDS_BYTES = 49152                    # csrc/inpaint.hip IP_LDS_BYTES
DESC_INTS = 16                       # csrc/inpaint.hip IP_DESC
MAX_FEATHER = 32                     # csrc/inpaint.hip IP_MAX_FEATHER
MEMBRANE_TILE = 32                   # csrc/membrane.hip MB_TILE: the smoother's tile side
MEMBRANE_COARSEST = 16               # csrc/membrane.hip MB_COARSEST: the largest side of a coarsest level
MEMBRANE_MAX_CYCLES = 44             # default of membrane_solve: twice the largest count seen, 22


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
    return window_of_box((int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1), H, W, R, context, feather)


def window_of_box(box, H, W, R, context=0.5, feather=8):
    """The window rule of ``plan_window`` for a hole box (ya, yb, xa, xb) (half-open) of an H x W image -> (y0, x0, ch, cw)."""
    ya, yb, xa, xb = (int(v) for v in box)
    H, W = int(H), int(W)
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


def build_gather_table(shapes, windows, R):
    """Host side of a ``gather_windows`` launch -> (int32 table, chunks, bands, LDS bytes): B descriptors of DESC_INTS ints (h, w, image
    offset, mask offset, y0, x0, ch, cw, horizontal bounds / coefficients / width, vertical bounds / coefficients / width, band rows,
    column chunk), then each distinct (in, R) pair's fixed-point table of ``resize.bicubic_coeffs`` once."""
    geo = _geometry(shapes, windows, 'gather_windows')
    R = int(R)
    if R < 1:
        raise ValueError(f'gather_windows: R must be >= 1 (got {R})')
    t = resize._Table(geo.shape[0], DESC_INTS)
    for i, g in enumerate(geo):
        ch, cw = int(g[6]), int(g[7])
        try:
            tb, cc, lds = resize._tiling(ch, R, R)
        except ValueError:
            raise ValueError(f'gather_windows: the {ch}-row window of image {i} is too tall to resample to {R} rows in one workgroup band') from None
        t.desc[i] = tuple(g) + t.place(cw, *resize.bicubic_coeffs(cw, R)) + t.place(ch, *resize.bicubic_coeffs(ch, R)) + (tb, cc)
        t.tile(-(-R // cc), -(-R // tb), lds)
    return t.finish('gather_windows', 12)


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
    t = resize._Table(geo.shape[0], DESC_INTS)

    def place(n_out):
        if n_out in t.placed:                                       # (the float32 rounding below is done once per size)
            return t.placed[n_out]
        bounds, w = bicubic_weights(R, n_out)
        return t.place(n_out, bounds, w.astype(np.float32).view(np.int32))

    for i, g in enumerate(geo):
        ch, cw = int(g[6]), int(g[7])
        tiling = _paste_tiling(ch, cw, R, feather)
        if tiling is None:
            raise ValueError(f'paste_back: image {i}: {R} rows resampled down to a {ch}-row window do not fit one workgroup band '
                             f'(a window that small is not pasted from a {R} x {R} output)')
        tb, cc, lds = tiling
        t.desc[i] = tuple(g) + place(cw) + place(ch) + (tb, cc)
        t.tile(-(-cw // cc), -(-ch // tb), lds)
    if t.chunks > 65535 or t.bands > 65535:
        raise ValueError('paste_back: a window has more than 65535 bands or chunks')
    return t.finish('paste_back', 32)


def _u8_flat(launch, t, name, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise _lib.ShgError(f'{what}: {name} must be a uint8 HIP tensor: libshgan_hip has no CPU path')
    return launch.req(t, name, dtype=torch.uint8).view(-1)


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


def _keyed(launch, what, owner, keys, packed_mask, B):
    """The (owner, keys) pair of a keyed paste-back, checked -> (owner flat uint8, keys int32 [B]), or (None, None) when neither is given."""
    if owner is None and keys is None:
        return None, None
    if owner is None or keys is None:
        raise _lib.ShgError(f'{what}: owner and keys are given together or not at all')
    owner = _u8_flat(launch, owner, 'owner', what)
    if owner.numel() != packed_mask.numel():
        raise _lib.ShgError(f'{what}: owner holds {owner.numel()} bytes, packed_mask {packed_mask.numel()}')
    try:
        keys = _host(keys).astype(np.int64).reshape(-1)
    except (TypeError, ValueError):
        raise _lib.ShgError(f'{what}: keys must be integers, one per window') from None
    if keys.shape[0] != B or (keys < 1).any() or (keys > 255).any():
        raise _lib.ShgError(f'{what}: keys must be {B} integers in 1..255 (got {keys.tolist()[:8]})')
    return owner, keys.astype(np.int32)


def paste_back(packed, packed_mask, shapes, windows, fake, k=1, feather=8, out=None, alpha_out=None, stream=None, owner=None, keys=None):
    """fake: float32 [B k, 3, R, R], the raw generator output, row n k + j = sample j of image n (``sample_many``'s layout) -> out uint8
    [k, len(packed)]: sample j of image n at image n's offset in row j.  ``out`` (made when None) starts as k copies of ``packed`` (one
    ``copy_``); the launch covers the windows only and stores nothing where the feather weight is 0, so every byte away from the hole is
    the original's.  ``feather`` in 0..32 (0: the hard composite).  ``alpha_out``: an optional uint8 tensor in packed-mask layout that
    receives the weight A (0 outside the windows).  One launch on ``stream`` (default: the current stream), no synchronisation.
    ``owner`` / ``keys`` (together): the keyed form for the windows of hole groups -- ``owner`` is ``owner_plane``'s uint8 plane, ``keys``
    host ints [B] in 1..255, and window b blends the holes whose owner byte is keys[b].  ``shapes`` / ``windows`` / ``fake`` rows are then
    per window (an image's row of ``shapes`` is repeated for each of its windows; the windows may overlap); ``packed_mask`` is still
    taken for the extent checks; ``alpha_out`` receives the sum of the windows' weights."""
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
    owner, keys = _keyed(launch, 'paste_back', owner, keys, packed_mask, B)
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
        if owner is None:
            check(_lib.get_lib().shg_inpaint_paste_u8(kernels._ptr(out), n, kernels._ptr(packed_mask), packed_mask.numel(), kernels._ptr(tab), tab.numel(),
                                                      kernels._ptr(fake), kernels._ptr(alpha_out), B, k, R, feather, chunks, bands, lds_bytes,
                                                      ctypes.c_void_p(st.cuda_stream)), 'paste_back')
        else:
            kd = _upload(keys, launch.dev)
            check(_lib.get_lib().shg_inpaint_paste_keyed_u8(kernels._ptr(out), n, kernels._ptr(owner), owner.numel(), kernels._ptr(kd), kernels._ptr(tab),
                                                            tab.numel(), kernels._ptr(fake), kernels._ptr(alpha_out), B, k, R, feather, chunks, bands,
                                                            lds_bytes, ctypes.c_void_p(st.cuda_stream)), 'paste_back')
    return out


def _r4(n):
    return (int(n) + 3) // 4 * 4


class MembranePlan:
    """Host side of a ``paste_back_membrane`` call (``membrane_plan``): ``grids`` int32 [B, 6] = (gy0, gx0, gh, gw, float offset, byte
    offset) per image, the solve grid in window coordinates and where its planes [k][gh][gw][3] (in ``g`` and ``field``) and its Omega
    bytes [gh][gw] start; ``table`` int32 [B k, 4] = (gh, gw, float offset, byte offset), the solver's problems, row n k + j = sample j of
    image n (the k samples of an image share its Omega offset); ``n`` int64 [B k], the shorter side of Omega's bounding box (the stop
    rule's n); ``g_elems`` / ``omega_bytes`` / ``ws_bytes``: the sizes of g and field (floats each), of omega and of the solver's
    workspace; ``max_h`` / ``max_w``: the largest grid sides."""
    __slots__ = ('grids', 'table', 'n', 'g_elems', 'omega_bytes', 'ws_bytes', 'max_h', 'max_w', 'k')


def membrane_workspace_bytes(P, max_h, max_w):
    """Bytes of ``membrane_solve``'s workspace for P problems of at most max_h x max_w: per problem the level-0 shadow (12 h w), one
    float per 32 x 32 tile, and per coarse level (h_l, w_l) = (ceil(h_{l-1} / 2), ceil(w_{l-1} / 2)) 36 h_l w_l + h_l w_l bytes (each
    array rounded up to 16 bytes) -- about 24.3 bytes per pixel of the largest grid."""
    n = int(_lib.get_lib().shg_membrane_workspace_bytes(int(P), int(max_h), int(max_w)))
    if n == 0:
        raise ValueError(f'membrane: P >= 1 and grid sides in 1..16384 are required (got {P}, {max_h} x {max_w})')
    return n


def membrane_plan(shapes, windows, feather, k, boxes=None):
    """-> ``MembranePlan``, integers only.  ``boxes``: host int [B, 4] = (ya, yb, xa, xb), a box of image n that holds every hole pixel of
    its window (``Inpainter`` passes the hole's bounding box).  Omega's bounding box is then the box clipped to the window, grown by
    ``feather`` and clipped again; the solve grid is that grown by one ring and clipped to the window.  Without ``boxes`` both are the
    whole window (the same membrane; more workspace)."""
    geo = _geometry(shapes, windows, 'membrane_plan')
    k, feather = int(k), int(feather)
    if k < 1 or not 0 <= feather <= MAX_FEATHER:
        raise ValueError(f'membrane_plan: k must be >= 1 and feather in 0..{MAX_FEATHER} (got {k}, {feather})')
    B = geo.shape[0]
    if boxes is not None:
        boxes = _host(boxes).astype(np.int64).reshape(-1, 4)
        if boxes.shape[0] != B:
            raise ValueError(f'membrane_plan: {B} images but {boxes.shape[0]} boxes')
    plan = MembranePlan()
    plan.k = k
    plan.grids, plan.table, plan.n = np.zeros((B, 6), np.int64), np.zeros((B * k, 4), np.int64), np.zeros(B * k, np.int64)
    foff = ooff = 0
    for i, (h, w, off, moff, y0, x0, ch, cw) in enumerate(geo):
        ya, yb, xa, xb = 0, ch, 0, cw
        if boxes is not None:
            ya, yb, xa, xb = max(boxes[i, 0] - y0, 0), min(boxes[i, 1] - y0, ch), max(boxes[i, 2] - x0, 0), min(boxes[i, 3] - x0, cw)
            if ya >= yb or xa >= xb:
                raise ValueError(f'membrane_plan: the box of image {i} does not meet its window')
            ya, yb, xa, xb = max(ya - feather, 0), min(yb + feather, ch), max(xa - feather, 0), min(xb + feather, cw)
        n = min(yb - ya, xb - xa)
        gy0, gy1, gx0, gx1 = max(ya - 1, 0), min(yb + 1, ch), max(xa - 1, 0), min(xb + 1, cw)
        gh, gw = gy1 - gy0, gx1 - gx0
        plan.grids[i] = (gy0, gx0, gh, gw, foff, ooff)
        for j in range(k):
            plan.table[i * k + j] = (gh, gw, foff + j * 3 * gh * gw, ooff)
            plan.n[i * k + j] = n
        foff, ooff = _r4(foff + 3 * k * gh * gw), _r4(ooff + gh * gw)
    if foff >= 2 ** 31:
        raise ValueError('membrane_plan: the solve grids of a call hold at most 2^31 floats')
    plan.g_elems, plan.omega_bytes = int(foff), int(ooff)
    plan.max_h, plan.max_w = int(plan.grids[:, 2].max()), int(plan.grids[:, 3].max())
    plan.ws_bytes = membrane_workspace_bytes(B * k, plan.max_h, plan.max_w)
    plan.grids, plan.table = plan.grids.astype(np.int32), plan.table.astype(np.int32)
    return plan


def _f32_flat(launch, t, name, what, elems):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= elems):
        raise _lib.ShgError(f'{what}: {name} must be a contiguous float32 HIP tensor of at least {elems} elements')
    launch._own(t, name)
    return t


def _membrane_operands(launch, what, packed, packed_mask, shapes, windows, plan, feather, R, owner=None, keys=None):
    packed = _u8_flat(launch, packed, 'packed', what)
    packed_mask = _u8_flat(launch, packed_mask, 'packed_mask', what)
    feather = int(feather)
    if not 0 <= feather <= MAX_FEATHER:
        raise _lib.ShgError(f'{what}: feather must lie in 0..{MAX_FEATHER} (got {feather})')
    geo = _geometry(shapes, windows, what)
    if not isinstance(plan, MembranePlan) or plan.grids.shape[0] != geo.shape[0]:
        raise _lib.ShgError(f'{what}: plan must be the MembranePlan of these {geo.shape[0]} images')
    _check_extent(geo, packed.numel(), packed_mask.numel(), what)
    owner, keys = _keyed(launch, what, owner, keys, packed_mask, geo.shape[0])
    table, chunks, bands, lds_bytes = build_paste_table(geo[:, :4], geo[:, 4:], R, feather)
    return packed, packed_mask, geo, table, chunks, bands, lds_bytes, owner, keys


def membrane_setup(packed, packed_mask, shapes, windows, fake, plan, g, field, omega, feather=8, stream=None, owner=None, keys=None):
    """First step of ``paste_back_membrane``: inside the solve grids of ``plan`` write ``g`` (float32 [plan.g_elems]: the resampled, scaled
    generator output, the bits ``paste_back`` blends), ``field`` (same layout: orig - g where the feather weight A is 0, 0 where A > 0)
    and ``omega`` (uint8 [plan.omega_bytes]: A > 0).  One launch.  ``owner`` / ``keys``: the keyed form, as ``paste_back``."""
    launch = kernels._Launch()
    B, k = plan.grids.shape[0] if isinstance(plan, MembranePlan) else 0, getattr(plan, 'k', 0)
    if not isinstance(fake, torch.Tensor) or fake.ndim != 4 or fake.shape[0] != B * k or fake.shape[1] != 3 or fake.shape[2] != fake.shape[3]:
        raise _lib.ShgError(f'membrane_setup: fake must be float32 [{B * k}, 3, R, R] (got {tuple(getattr(fake, "shape", ()))})')
    R = fake.shape[2]
    packed, packed_mask, geo, table, chunks, bands, lds_bytes, owner, keys = _membrane_operands(launch, 'membrane_setup', packed, packed_mask, shapes,
                                                                                                windows, plan, feather, R, owner, keys)
    fake = launch.req(fake, 'fake')
    g = _f32_flat(launch, g, 'g', 'membrane_setup', plan.g_elems)
    field = _f32_flat(launch, field, 'field', 'membrane_setup', plan.g_elems)
    if not (isinstance(omega, torch.Tensor) and omega.is_cuda and omega.dtype == torch.uint8 and omega.is_contiguous() and omega.numel() >= plan.omega_bytes):
        raise _lib.ShgError(f'membrane_setup: omega must be a contiguous uint8 HIP tensor of at least {plan.omega_bytes} bytes')
    launch._own(omega, 'omega')
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    with launch, torch.cuda.stream(st):
        tab, grids = _upload(table, launch.dev), _upload(plan.grids.reshape(-1), launch.dev)
        tail = (kernels._ptr(tab), tab.numel(), kernels._ptr(grids), kernels._ptr(fake), kernels._ptr(g), kernels._ptr(field), g.numel(),
                kernels._ptr(omega), omega.numel(), B, k, R, int(feather), chunks, bands, lds_bytes, ctypes.c_void_p(st.cuda_stream))
        if owner is None:
            check(_lib.get_lib().shg_inpaint_membrane_setup_f32(kernels._ptr(packed), packed.numel(), kernels._ptr(packed_mask), packed_mask.numel(), *tail),
                  'membrane_setup')
        else:
            kd = _upload(keys, launch.dev)
            check(_lib.get_lib().shg_inpaint_membrane_setup_keyed_f32(kernels._ptr(packed), packed.numel(), kernels._ptr(owner), owner.numel(),
                                                                      kernels._ptr(kd), *tail), 'membrane_setup')


def membrane_solve(field, omega, table, tol=0.25, max_cycles=None, info_out=None, stream=None, n=None, ws=None):
    """The masked Laplace solver alone.  ``table``: host int [P, 4] = (h, w, float offset into ``field``, byte offset into ``omega``);
    problem p is field float32 [h][w][3] with omega uint8 [h][w] (non-zero = unknown); neighbours outside the h x w grid count as 0; the
    problems' slices of ``field`` must not overlap (several may share an omega).  On return ``field`` holds the membrane c in Omega and is
    untouched elsewhere.  Stop rule: the residual's max norm over Omega and the three channels <= 8 tol / (n + 1)^2, ``n`` (host int [P];
    default min(h, w)) at least the shorter side of Omega's bounding box: then |c - c*| <= tol everywhere (state 1).  -> info, device
    int32 [P, 3] = (cycles run, bits of the last residual norm as float32, state 1 certified / 2 stalled at the float32 floor / 0 out of
    ``max_cycles``, default ``MEMBRANE_MAX_CYCLES``).  ``ws``: an optional uint8 workspace of ``membrane_workspace_bytes`` bytes, its
    contents irrelevant.  A fixed sequence of launches on ``stream``; nothing is synchronised."""
    launch = kernels._Launch()
    table = _host(table).astype(np.int64).reshape(-1, 4)
    P = table.shape[0]
    if P < 1 or (table[:, :2] < 1).any() or (table[:, 2:] < 0).any() or np.abs(table).max() >= 2 ** 31:
        raise _lib.ShgError('membrane_solve: table must be int [P, 4] = (h, w, field offset, omega offset) with h, w >= 1 and offsets >= 0')
    need_f, need_o = int((table[:, 2] + 3 * table[:, 0] * table[:, 1]).max()), int((table[:, 3] + table[:, 0] * table[:, 1]).max())
    field = _f32_flat(launch, field, 'field', 'membrane_solve', need_f)
    if not (isinstance(omega, torch.Tensor) and omega.is_cuda and omega.dtype == torch.uint8 and omega.is_contiguous() and omega.numel() >= need_o):
        raise _lib.ShgError(f'membrane_solve: omega must be a contiguous uint8 HIP tensor of at least {need_o} bytes')
    launch._own(omega, 'omega')
    order = np.argsort(table[:, 2], kind='stable')
    ends = (table[:, 2] + 3 * table[:, 0] * table[:, 1])[order]
    if (ends[:-1] > table[order[1:], 2]).any():
        raise _lib.ShgError('membrane_solve: the problems overlap in field')
    n = table[:, :2].min(axis=1) if n is None else _host(n).astype(np.int64).reshape(-1)
    if n.shape[0] != P or (n < 1).any() or not float(tol) > 0.0:
        raise _lib.ShgError(f'membrane_solve: tol > 0 and one n >= 1 per problem are required (got tol = {tol}, {n.shape[0]} values of n)')
    res_tol = (8.0 * float(tol) / (n.astype(np.float64) + 1.0) ** 2).astype(np.float32)
    max_cycles = MEMBRANE_MAX_CYCLES if max_cycles is None else int(max_cycles)
    if not 0 <= max_cycles <= 1024:
        raise _lib.ShgError(f'membrane_solve: max_cycles must lie in 0..1024 (got {max_cycles})')
    max_h, max_w = int(table[:, 0].max()), int(table[:, 1].max())
    ws_bytes = membrane_workspace_bytes(P, max_h, max_w)
    if ws is not None:
        if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= ws_bytes):
            raise _lib.ShgError(f'membrane_solve: ws must be a contiguous uint8 HIP tensor of at least {ws_bytes} bytes')
        launch._own(ws, 'ws')
    if info_out is not None:
        if not (isinstance(info_out, torch.Tensor) and info_out.is_cuda and info_out.dtype == torch.int32 and info_out.is_contiguous()
                and tuple(info_out.shape) == (P, 3)):
            raise _lib.ShgError(f'membrane_solve: info_out must be a contiguous int32 HIP tensor [{P}, 3]')
        launch._own(info_out, 'info_out')
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    with launch, torch.cuda.stream(st):
        tab = _upload(table.astype(np.int32).reshape(-1), launch.dev)
        rt = _upload(res_tol, launch.dev)
        if ws is None:
            ws = launch.new((ws_bytes,), torch.uint8)
        info = launch.new((P, 3), torch.int32) if info_out is None else info_out
        check(_lib.get_lib().shg_membrane_solve_f32(kernels._ptr(field), field.numel(), kernels._ptr(omega), omega.numel(), kernels._ptr(tab), P,
                                                    kernels._ptr(rt), max_cycles, max_h, max_w, kernels._ptr(ws), ws.numel(), kernels._ptr(info),
                                                    ctypes.c_void_p(st.cuda_stream)), 'membrane_solve')
    return info


def membrane_paste(packed_mask, shapes, windows, plan, g, field, out, R, feather=8, alpha_out=None, stream=None, owner=None, keys=None):
    """Last step of ``paste_back_membrane``: ``paste_back``'s blend with clamp(g + c, 0, 255) in place of g (``field`` holds c in Omega),
    into ``out`` uint8 [k, bytes], every row a copy of the packed originals on entry.  One launch.  ``owner`` / ``keys``: the keyed form,
    as ``paste_back``."""
    launch = kernels._Launch()
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.ndim == 2 and out.is_contiguous()
            and out.shape[0] == getattr(plan, 'k', 0)):
        raise _lib.ShgError(f'membrane_paste: out must be a contiguous uint8 HIP tensor [{getattr(plan, "k", 0)}, bytes]')
    k, n = out.shape
    _, packed_mask, geo, table, chunks, bands, lds_bytes, owner, keys = _membrane_operands(launch, 'membrane_paste', out.view(-1)[:n], packed_mask,
                                                                                           shapes, windows, plan, feather, int(R), owner, keys)
    g = _f32_flat(launch, g, 'g', 'membrane_paste', plan.g_elems)
    field = _f32_flat(launch, field, 'field', 'membrane_paste', plan.g_elems)
    if alpha_out is not None:
        if not (isinstance(alpha_out, torch.Tensor) and alpha_out.is_cuda and alpha_out.dtype == torch.uint8 and alpha_out.is_contiguous()
                and alpha_out.numel() == packed_mask.numel()):
            raise _lib.ShgError(f'membrane_paste: alpha_out must be a contiguous uint8 HIP tensor of {packed_mask.numel()} bytes')
        launch._own(alpha_out, 'alpha_out')
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    with launch, torch.cuda.stream(st):
        tab, grids = _upload(table, launch.dev), _upload(plan.grids.reshape(-1), launch.dev)
        if alpha_out is not None:
            alpha_out.zero_()
        tail = (kernels._ptr(tab), tab.numel(), kernels._ptr(grids), kernels._ptr(g), kernels._ptr(field), g.numel(), kernels._ptr(alpha_out),
                geo.shape[0], k, int(R), int(feather), chunks, bands, lds_bytes, ctypes.c_void_p(st.cuda_stream))
        if owner is None:
            check(_lib.get_lib().shg_inpaint_membrane_paste_u8(kernels._ptr(out), n, kernels._ptr(packed_mask), packed_mask.numel(), *tail), 'membrane_paste')
        else:
            kd = _upload(keys, launch.dev)
            check(_lib.get_lib().shg_inpaint_membrane_paste_keyed_u8(kernels._ptr(out), n, kernels._ptr(owner), owner.numel(), kernels._ptr(kd), *tail),
                  'membrane_paste')
    return out


def paste_back_membrane(packed, packed_mask, shapes, windows, fake, k=1, feather=8, tol=0.25, out=None, alpha_out=None, info_out=None, stream=None,
                        boxes=None, max_cycles=None, owner=None, keys=None):
    """``paste_back`` with the gradient-domain blend: same operands, same result layout, the same bytes wherever the feather weight is 0.
    In Omega = {A > 0} the blended value is clamp(g + c, 0, 255) instead of g, c the membrane of the module's docstring, solved to ``tol``
    grey levels where float32 allows (``info_out``, int32 [B k, 3], receives ``membrane_solve``'s info; state 2 = the float32 floor, see
    INTEGRATION section S).  ``boxes``: see ``membrane_plan``.  Workspaces (g, field, omega, the solver's) are allocated per call.
    Launches on ``stream`` (default: the current stream), no synchronisation.  ``owner`` / ``keys``: the keyed form, as ``paste_back``
    (rows per window; ``boxes`` are then the groups' hole boxes and ``info_out`` has a row per (window, sample))."""
    launch = kernels._Launch()
    packed = _u8_flat(launch, packed, 'packed', 'paste_back_membrane')
    k, feather = int(k), int(feather)
    if k < 1 or not 0 <= feather <= MAX_FEATHER:
        raise _lib.ShgError(f'paste_back_membrane: k must be >= 1 and feather in 0..{MAX_FEATHER} (got {k}, {feather})')
    geo = _geometry(shapes, windows, 'paste_back_membrane')
    B = geo.shape[0]
    if not isinstance(fake, torch.Tensor) or fake.ndim != 4 or fake.shape[0] != B * k or fake.shape[1] != 3 or fake.shape[2] != fake.shape[3]:
        raise _lib.ShgError(f'paste_back_membrane: fake must be float32 [{B * k}, 3, R, R] (got {tuple(getattr(fake, "shape", ()))})')
    n = packed.numel()
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (k, n) and out.is_contiguous()):
            raise _lib.ShgError(f'paste_back_membrane: out must be a contiguous uint8 HIP tensor [{k}, {n}]')
        if out.data_ptr() < packed.data_ptr() + n and packed.data_ptr() < out.data_ptr() + k * n:
            raise _lib.ShgError('paste_back_membrane: out overlaps packed')
        launch._own(out, 'out')
    plan = membrane_plan(geo[:, :4], geo[:, 4:], feather, k, boxes)
    if owner is not None or keys is not None:                                       # (refused before anything is written)
        pm = _u8_flat(launch, packed_mask, 'packed_mask', 'paste_back_membrane')
        _check_extent(geo, n, pm.numel(), 'paste_back_membrane')
        _keyed(launch, 'paste_back_membrane', owner, keys, pm, B)
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    with launch, torch.cuda.stream(st):
        g = launch.new((plan.g_elems,), torch.float32)
        field = launch.new((plan.g_elems,), torch.float32)
        omega = launch.new((plan.omega_bytes,), torch.uint8)
        ws = launch.new((plan.ws_bytes,), torch.uint8)
        if out is None:
            out = launch.new((k, n), torch.uint8)
        out.copy_(packed.view(1, n).expand(k, n))
        membrane_setup(packed, packed_mask, geo[:, :4], geo[:, 4:], fake, plan, g, field, omega, feather, st, owner, keys)
        membrane_solve(field, omega, plan.table, tol, max_cycles, info_out, st, plan.n, ws)
        membrane_paste(packed_mask, geo[:, :4], geo[:, 4:], plan, g, field, out, fake.shape[2], feather, alpha_out, st, owner, keys)
    return out


# ------------------------------------------------------------------------------------------------
# hole groups: one window per group of holes (csrc/hole_label.hip)
# ------------------------------------------------------------------------------------------------

def hole_label_tile():
    """The side of the tile one workgroup of ``label_holes`` labels in LDS (csrc/hole_label.hip HL_TILE)."""
    return int(_lib.get_lib().shg_hole_label_tile())


def _shapes4(shapes, n_mask, what):
    """-> int64 [B, 4] = (h, w, image offset, mask offset), every mask inside the ``n_mask`` bytes."""
    shapes = _host(shapes).astype(np.int64)
    shapes = shapes.reshape(-1, 4 if shapes.ndim == 2 and shapes.shape[1] == 4 else 3)
    if shapes.shape[0] < 1:
        raise _lib.ShgError(f'{what}: at least one image is required')
    if shapes.shape[1] == 3:
        px = shapes[:, 0] * shapes[:, 1]
        shapes = np.concatenate([shapes, (np.cumsum(px) - px)[:, None]], axis=1)
    for i, (h, w, off, moff) in enumerate(shapes):
        if h < 1 or w < 1 or moff < 0 or moff + h * w > n_mask:
            raise _lib.ShgError(f'{what}: image {i} ({h}x{w}, mask at {moff}) does not lie inside packed_mask ({n_mask} bytes)')
    return shapes


class HoleLabels:
    """What ``label_holes`` leaves on the device: ``labels`` int32 [mask bytes] (the root y w + x of the pixel's group, -1 outside D),
    ``state`` int32 [max_components + 1, 8]: row 0 = (groups found, flags, ...), rows 1.. = (image, root, ya, yb, xa, xb, hole pixels, 0) in
    no particular order; ``shapes`` (host int64 [B, 4]), ``feather`` and ``max_components`` as given."""
    __slots__ = ('labels', 'state', 'shapes', 'feather', 'max_components')


def label_holes(packed_mask, shapes, feather, max_components=4096, stream=None):
    """Group the holes of a packed batch of masks on the device -> ``HoleLabels``.  With r = feather + 1: D = the pixels within Chebyshev
    distance r of a hole pixel of the same image, a group = an 8-connected component of D, its root the smallest y w + x of its pixels
    (INTEGRATION section T).  A memset and at most four launches on ``stream`` (default: the current stream); nothing is synchronised.
    Workspace: 4 bytes per mask pixel for the labels and one int32 scratch plane of the same size, freed on return (``owner_plane`` takes
    another such plane and 1 byte per pixel for its result); 32 bytes per component of capacity."""
    launch = kernels._Launch()
    packed_mask = _u8_flat(launch, packed_mask, 'packed_mask', 'label_holes')
    feather, max_components = int(feather), int(max_components)
    if not 0 <= feather <= MAX_FEATHER or not 1 <= max_components <= 2 ** 24:
        raise _lib.ShgError(f'label_holes: feather in 0..{MAX_FEATHER} and max_components in 1..2^24 are required (got {feather}, {max_components})')
    n = packed_mask.numel()
    shapes = _shapes4(shapes, n, 'label_holes')
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    lbl = HoleLabels()
    lbl.shapes, lbl.feather, lbl.max_components = shapes, feather, max_components
    with launch, torch.cuda.stream(st):
        sh = _upload(shapes.astype(np.int32).reshape(-1), launch.dev)
        lbl.labels = launch.new((n,), torch.int32)
        scratch = launch.new((n,), torch.int32)
        lbl.state = launch.new((max_components + 1, 8), torch.int32)
        check(_lib.get_lib().shg_hole_label_i32(kernels._ptr(packed_mask), n, kernels._ptr(sh), shapes.shape[0], int(shapes[:, 0].max()),
                                                int(shapes[:, 1].max()), feather + 1, max_components, kernels._ptr(lbl.labels), kernels._ptr(scratch),
                                                kernels._ptr(lbl.state[1:]), kernels._ptr(lbl.state), ctypes.c_void_p(st.cuda_stream)), 'label_holes')
    return lbl


def fetch_components(lbl):
    """The one small device-to-host copy of a labelling (it synchronises) -> int64 [C, 7] = (image, root, ya, yb, xa, xb, hole pixels)
    sorted by (image, root).  More groups than the capacity raise ``ValueError``; a loop cap hit on the device raises ``ShgError``."""
    if not isinstance(lbl, HoleLabels):
        raise _lib.ShgError('fetch_components: a HoleLabels object (label_holes) is required')
    state = lbl.state.cpu().numpy().astype(np.int64)
    found, flags = int(state[0, 0]), int(state[0, 1])
    if flags & 2:
        raise _lib.ShgError('label_holes: a find / union loop ran into its iteration cap on the device; the labels are not usable')
    if flags & 1 or found > lbl.max_components:
        raise ValueError(f'label_holes: the masks hold {found} hole groups, more than max_components = {lbl.max_components}')
    comps = state[1:1 + found, :7]
    return comps[np.lexsort((comps[:, 1], comps[:, 0]))]


class WindowPlan:
    """``plan_windows``' result, one entry per window in (image, key) order: ``image`` int64 [N], ``key`` int64 [N] (1..255), ``windows``
    int64 [N, 4] = (y0, x0, ch, cw), ``boxes`` int64 [N, 4] = (ya, yb, xa, xb) of the window's hole pixels; ``table`` int64 [C, 3] =
    (image, root, key) over every group."""
    __slots__ = ('image', 'key', 'windows', 'boxes', 'table')


def plan_windows(components, shapes, R, context=0.5, feather=8, max_windows=16):
    """components: int [C, 7] (``fetch_components``) -> ``WindowPlan``, integers only.  Within an image the groups take the keys 1, 2, ...
    in order of increasing root and each its own window: ``plan_window``'s rule (``window_of_box``) on the group's hole box.  An image
    with more than ``max_windows`` (at most 255) groups is served as by ``plan_window``: one window over all its holes, every group key 1."""
    max_windows = int(max_windows)
    if not 1 <= max_windows <= 255:
        raise ValueError(f'plan_windows: max_windows must lie in 1..255 (got {max_windows})')
    comps = _host(components).astype(np.int64).reshape(-1, 7)
    shapes = _host(shapes).astype(np.int64)
    shapes = shapes.reshape(-1, shapes.shape[-1] if shapes.ndim == 2 else 3)
    if comps.shape[0] and (comps[:, 0].min() < 0 or comps[:, 0].max() >= shapes.shape[0]):
        raise ValueError(f'plan_windows: a component names an image outside 0..{shapes.shape[0] - 1}')
    comps = comps[np.lexsort((comps[:, 1], comps[:, 0]))]
    image, key, windows, boxes, table = [], [], [], [], []
    for i in np.unique(comps[:, 0]):
        rows = comps[comps[:, 0] == i]
        H, W = int(shapes[i, 0]), int(shapes[i, 1])
        if rows.shape[0] > max_windows:
            box = (int(rows[:, 2].min()), int(rows[:, 3].max()), int(rows[:, 4].min()), int(rows[:, 5].max()))
            image.append(i), key.append(1), boxes.append(box), windows.append(window_of_box(box, H, W, R, context, feather))
            table += [(i, int(r[1]), 1) for r in rows]
            continue
        for j, r in enumerate(rows):
            box = tuple(int(v) for v in r[2:6])
            image.append(i), key.append(j + 1), boxes.append(box), windows.append(window_of_box(box, H, W, R, context, feather))
            table.append((i, int(r[1]), j + 1))
    plan = WindowPlan()
    plan.image, plan.key = np.array(image, np.int64), np.array(key, np.int64)
    plan.windows, plan.boxes = np.array(windows, np.int64).reshape(-1, 4), np.array(boxes, np.int64).reshape(-1, 4)
    plan.table = np.array(table, np.int64).reshape(-1, 3)
    return plan


def owner_plane(lbl, packed_mask, shapes, table, stream=None):
    """-> uint8 tensor in packed-mask layout on the device: 0 at known pixels, at a hole pixel the key its group has in ``table`` (host int
    [C, 3] = (image, root, key in 1..255), ``plan_windows``' table; 0 for a group it does not name).  Three launches, nothing is
    synchronised.  Workspace: one int32 scratch plane (4 bytes per mask pixel), freed on return, and the result's 1 byte per pixel."""
    launch = kernels._Launch()
    if not isinstance(lbl, HoleLabels):
        raise _lib.ShgError('owner_plane: a HoleLabels object (label_holes) is required')
    packed_mask = _u8_flat(launch, packed_mask, 'packed_mask', 'owner_plane')
    n = packed_mask.numel()
    launch._own(lbl.labels, 'labels')
    shapes = _shapes4(shapes, n, 'owner_plane')
    if lbl.labels.numel() != n or not np.array_equal(shapes, lbl.shapes):
        raise _lib.ShgError('owner_plane: the labels belong to other masks (sizes or shapes differ)')
    table = _host(table).astype(np.int64).reshape(-1, 3)
    if table.shape[0] and (table[:, 0].min() < 0 or table[:, 0].max() >= shapes.shape[0] or table[:, 1].min() < 0 or table[:, 2].min() < 1
                           or table[:, 2].max() > 255 or (table[:, 1] >= (shapes[:, 0] * shapes[:, 1])[np.clip(table[:, 0], 0, shapes.shape[0] - 1)]).any()):
        raise _lib.ShgError('owner_plane: table rows must be (image, root inside the image, key in 1..255)')
    st = stream if stream is not None else torch.cuda.current_stream(launch.dev)
    with launch, torch.cuda.stream(st):
        sh = _upload(shapes.astype(np.int32).reshape(-1), launch.dev)
        tab = _upload(table.astype(np.int32).reshape(-1), launch.dev) if table.shape[0] else None
        scratch = launch.new((n,), torch.int32)
        owner = launch.new((n,), torch.uint8)
        check(_lib.get_lib().shg_hole_owner_u8(kernels._ptr(packed_mask), n, kernels._ptr(sh), shapes.shape[0], int(shapes[:, 0].max()),
                                               int(shapes[:, 1].max()), kernels._ptr(lbl.labels), kernels._ptr(tab), table.shape[0], kernels._ptr(scratch),
                                               kernels._ptr(owner), ctypes.c_void_p(st.cuda_stream)), 'owner_plane')
    return owner


class Inpainter:
    """``Inpainter(G, resolution, device)(images, masks)`` -> the images with their holes filled.

    images: uint8 [h, w, 3] arrays of any sizes; masks: [h, w] arrays, 0 = hole.  Per image the window of ``plan_window`` is gathered at
    ``resolution``, assembled (``eval_harness.assemble_input``), run through ``G`` (``G.sample_many`` when ``samples > 1``) and pasted
    back with a feather of ``feather`` native pixels.  The result is a list in the order of the inputs: one [h, w, 3] uint8 array per
    image, or [samples, h, w, 3] when ``samples > 1``.  An image without a hole comes back as a copy and never reaches the device.  Images
    are processed in chunks of ``batch``; a chunk is one upload, the launches (no host synchronisation between them) and one
    device-to-host copy.  ``gather_fn`` / ``paste_fn`` (the signatures of ``gather_windows`` / ``paste_back``) and ``G`` can be replaced,
    so the flow also runs on the host with reference functions and a stand-in generator.  ``blend``: 'feather' (``paste_back``) or
    'membrane' (``paste_back_membrane``, with the holes' bounding boxes as ``boxes``; ``info`` then holds the solver's info of the last
    call, one int32 [images samples, 3] array per chunk, fetched with a second small copy).  A given ``paste_fn`` is called as
    ``paste_back`` is, whatever ``blend`` says.

    ``windows``: 'one' (the default: one window over all holes of an image) or 'per_hole': the holes of an image are grouped
    (``label_holes``: holes nearer than 2 (feather + 1) known pixels share a group) and every group gets its own window
    (``plan_windows``; an image with more than ``max_windows`` groups falls back to one window).  Per chunk: upload, label,
    ``fetch_components`` (ONE EXTRA host synchronisation per chunk, a copy of 32 bytes per component of capacity), plan, ``owner_plane``,
    one gather over all windows of the chunk, ``G`` on at most ``batch`` windows at a time, one keyed paste over all windows, the one
    device-to-host copy.  All windows of image i share image i's latents, so a result depends neither on the chunking nor on ``batch``;
    with ``blend='membrane'`` the ``boxes`` are the groups' hole boxes and ``info`` has a row per (window, sample).  ``windows_`` keeps the
    last call's plan: a list of (image index of the call, key, (y0, x0, ch, cw), (ya, yb, xa, xb)).  ``label_fn(packed_mask, shapes,
    feather)`` -> int [C, 7] and ``owner_fn(packed_mask, shapes, table, feather)`` -> uint8 plane replace the device labelling (both or
    neither), as ``gather_fn`` / ``paste_fn`` replace theirs."""

    def __init__(self, G, resolution, device, context=0.5, feather=8, noise_mode='const', batch=16, gather_fn=None, paste_fn=None, blend='feather',
                 windows='one', max_windows=16, label_fn=None, owner_fn=None):
        if int(batch) < 1 or not 0 <= int(feather) <= MAX_FEATHER or int(resolution) < 1:
            raise ValueError(f'Inpainter: batch >= 1, resolution >= 1 and feather in 0..{MAX_FEATHER} are required')
        if blend not in ('feather', 'membrane'):
            raise ValueError(f"Inpainter: blend must be 'feather' or 'membrane' (got {blend!r})")
        if windows not in ('one', 'per_hole') or not 1 <= int(max_windows) <= 255 or (label_fn is None) != (owner_fn is None):
            raise ValueError(f"Inpainter: windows must be 'one' or 'per_hole' (got {windows!r}), max_windows in 1..255, and label_fn / owner_fn "
                             'are given together or not at all')
        self.windows, self.max_windows, self.label_fn, self.owner_fn, self.windows_ = windows, int(max_windows), label_fn, owner_fn, []
        self.blend, self.info = blend, []
        self._own_membrane = blend == 'membrane' and paste_fn is None
        self.G, self.resolution, self.device = G, int(resolution), torch.device(device)
        self.context, self.feather, self.noise_mode, self.batch = float(context), int(feather), noise_mode, int(batch)
        self.gather_fn = gather_windows if gather_fn is None else gather_fn
        self.paste_fn = (paste_back_membrane if blend == 'membrane' else paste_back) if paste_fn is None else paste_fn

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
            if self._own_membrane:
                boxes = []
                for mk in masks:
                    hole = np.asarray(mk) == 0
                    rows, cols = np.flatnonzero(hole.any(axis=1)), np.flatnonzero(hole.any(axis=0))
                    boxes.append((rows[0], rows[-1] + 1, cols[0], cols[-1] + 1))
                launch = kernels._Launch()
                launch._own(packed, 'packed')
                info = launch.new((len(images) * samples, 3), torch.int32)
                out = self.paste_fn(packed, packed_mask, shapes, windows, fake.float(), k=samples, feather=self.feather, info_out=info, boxes=boxes)
            else:
                out = self.paste_fn(packed, packed_mask, shapes, windows, fake.float(), k=samples, feather=self.feather)
        host = out.cpu().numpy()                                                    # the chunk's one device-to-host copy (it synchronises)
        if self._own_membrane:
            self.info.append(info.cpu().numpy())
        res = []
        for (h, w, off) in shapes[:, :3]:
            a = host[:, off:off + 3 * h * w].reshape(samples, h, w, 3)
            res.append(a.copy() if samples > 1 else a[0].copy())
        return res

    def _chunk_per_hole(self, images, masks, ids, z, samples):
        """One chunk of ``windows='per_hole'``; ``ids``: the images' indices in the call (for ``windows_``); z: [images, samples, z_dim]."""
        packed, shapes = resize.pack_images(images)
        packed_mask, moffs = pack_masks(masks)
        shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
        dev = self.device
        if dev.type == 'cuda':
            packed, packed_mask = packed.pin_memory().to(dev, non_blocking=True), packed_mask.pin_memory().to(dev, non_blocking=True)
        with torch.no_grad():
            if self.label_fn is None:
                lbl = label_holes(packed_mask, shapes, self.feather)
                comps = fetch_components(lbl)                                           # the chunk's extra synchronisation
            else:
                comps = self.label_fn(packed_mask, shapes, self.feather)
            plan = plan_windows(comps, shapes, self.resolution, self.context, self.feather, self.max_windows)
            if self.label_fn is None:
                owner = owner_plane(lbl, packed_mask, shapes, plan.table)
            else:
                owner = self.owner_fn(packed_mask, shapes, plan.table, self.feather)
            N = plan.image.shape[0]
            self.windows_ += [(ids[int(i)], int(k), tuple(int(v) for v in w), tuple(int(v) for v in b))
                              for i, k, w, b in zip(plan.image, plan.key, plan.windows, plan.boxes)]
            wshapes = shapes[plan.image]
            real, m = self.gather_fn(packed, packed_mask, wshapes, plan.windows, self.resolution)
            x = eval_harness.assemble_input(real, m)
            zw = z[torch.from_numpy(plan.image)].to(dev)
            parts = []
            for s in range(0, N, self.batch):
                xs, zs = x[s:s + self.batch], zw[s:s + self.batch]
                if samples > 1:
                    f = self.G.sample_many(xs, zs, None, noise_mode=self.noise_mode)
                    f = f.reshape((-1,) + tuple(f.shape[2:]))
                else:
                    f = self.G(x=xs, z=zs[:, 0], c=zs[:, 0, :0], noise_mode=self.noise_mode)
                parts.append(f.float())
            fake = torch.cat(parts) if len(parts) > 1 else parts[0]
            kw = dict(k=samples, feather=self.feather, owner=owner, keys=plan.key)
            if self._own_membrane:
                launch = kernels._Launch()
                launch._own(packed, 'packed')
                info = launch.new((N * samples, 3), torch.int32)
                kw.update(info_out=info, boxes=plan.boxes)
            out = self.paste_fn(packed, packed_mask, wshapes, plan.windows, fake, **kw)
        host = out.cpu().numpy()                                                    # the chunk's one device-to-host copy of images
        if self._own_membrane:
            self.info.append(info.cpu().numpy())
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
        per_hole = self.windows == 'per_hole'
        if per_hole:                                                                # (the windows are planned per chunk, from the device's groups)
            windows = [True if (np.asarray(mk) == 0).any() else None for mk in masks]
        else:
            windows = [plan_window(mk, self.resolution, self.context, self.feather) for mk in masks]
        todo = [i for i, wnd in enumerate(windows) if wnd is not None]
        if z is not None:
            z = torch.as_tensor(z, dtype=torch.float32).cpu()
            z = z[:, None] if z.ndim == 2 else z
            if z.ndim != 3 or z.shape[0] != len(images) or z.shape[1] != samples:
                raise ValueError(f'Inpainter: z must be [{len(images)}, z_dim] or [{len(images)}, {samples}, z_dim] (got {tuple(z.shape)})')
        result = [None] * len(images)
        self.info, self.windows_ = [], []
        for i, wnd in enumerate(windows):
            if wnd is None:
                result[i] = np.broadcast_to(images[i], (samples,) + images[i].shape).copy() if samples > 1 else images[i].copy()
        for s in range(0, len(todo), self.batch):
            ids = todo[s:s + self.batch]
            zc = torch.cat([self._latents(1, samples, seed, i) for i in ids]) if z is None else z[ids]
            if per_hole:
                for i, r in zip(ids, self._chunk_per_hole([images[i] for i in ids], [masks[i] for i in ids], ids, zc, samples)):
                    result[i] = r
                continue
            for i, r in zip(ids, self._chunk([images[i] for i in ids], [masks[i] for i in ids], [windows[i] for i in ids], zc, samples)):
                result[i] = r
        return result
