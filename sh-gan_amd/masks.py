"""On-device synthesis of the freeform masks of the eval / training loops (reference:
lib/data_factory/ds_ffhq.py:145-217 ``RandomBrush`` / ``RandomMask``).

Split of the work:
  * HOST (this file): the random draws, made from numpy's global ``RandomState`` in exactly the reference's order, and the
    geometry that depends only on them -- every mask becomes a short list of integer primitives (rectangles to punch,
    thick-line quads, discs, the two flip decisions);
  * DEVICE (csrc/mask_raster.hip, ``shg_mask_raster_f32``): rasterisation of the primitives, the AND of the two layers, the
    hole count, and -- through ``shg_assemble_input_f32`` -- the generator input ``cat([mask-0.5, real*mask])`` without a
    host round trip.

Bit-exactness: the reference draws with Pillow (``ImageDraw.line(width=..)`` + ``ImageDraw.ellipse``), so Pillow's
rasteriser is the specification.  The quad of a thick segment and its scan-line fill are restated from Pillow's
``ImagingDrawWideLine`` / ``polygon_generic`` (float32 edge slopes, the ROUND_UP / ROUND_DOWN span rule, the corner
joining); disc spans are read once per radius from Pillow itself (translation invariant, 18 radii).  The golden masks
of tests/golden/integer_paths.npz pin the result.

The rejection loop of ``RandomMask`` (re-draw while the hole ratio is outside ``hole_range``) needs the rasterised mask:
masks are generated speculatively in batches, the device returns the hole counts, and on a rejection the global RNG is
rewound to the state after the rejected attempt and the rest of the batch is drawn again -- the RNG stream, and so the
masks, equal the reference's sequential loop."""
import math

import numpy as np
import torch

from . import _lib, kernels
from ._lib import check

RECT, DISC, QUAD, EDGE, POINT, SEG = 0, 1, 2, 3, 4, 5
REC = 8                                   # int32 words per primitive record
MAX_HALF = 32                             # disc radii served by the span table


def _round_up(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 0.0, np.floor(f + 0.5), -np.floor(np.abs(f) + 0.5)).astype(np.int64)


def _round_down(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 0.0, np.ceil(f - 0.5), -np.ceil(np.abs(f) - 0.5)).astype(np.int64)


def _edge_records(xa, ya, xb, yb):
    """[n] edges (xa,ya)->(xb,yb) -> [n, 8] EDGE records (Pillow ``add_edge``): slope in float32."""
    n = len(xa)
    rec = np.zeros((n, REC), dtype=np.int32)
    rec[:, 0] = EDGE
    rec[:, 1], rec[:, 2] = xa, ya
    rec[:, 3], rec[:, 4] = np.minimum(ya, yb), np.maximum(ya, yb)
    dy = (yb - ya).astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        dx = np.where(dy != 0, (xb - xa).astype(np.float32) / np.where(dy != 0, dy, np.float32(1)), np.float32(0)).astype(np.float32)
    rec[:, 5] = dx.view(np.int32)
    rec[:, 6], rec[:, 7] = np.minimum(xa, xb), np.maximum(xa, xb)
    return rec


def thick_polyline_records(path, width, s):
    """Records of ``ImageDraw.line(path, width=width)`` on an s x s canvas: one QUAD (+ 4 EDGE) per segment
    (``ImagingDrawWideLine``), a POINT for a zero-length segment."""
    p = np.asarray(path, dtype=np.int64)
    x0, y0, x1, y1 = p[:-1, 0], p[:-1, 1], p[1:, 0], p[1:, 1]
    dx, dy = x1 - x0, y1 - y0
    out = []
    zero = (dx == 0) & (dy == 0)
    big = np.hypot(dx.astype(np.float64), dy.astype(np.float64))
    big = np.where(zero, 1.0, big)
    small = (width - 1) / 2.0
    rmax, rmin = float(_round_up(small)) / big, float(_round_down(small)) / big
    dxmin, dxmax = _round_down(rmin * dy), _round_down(rmax * dy)
    dymin, dymax = _round_up(rmin * dx), _round_up(rmax * dx)
    vx = np.stack([x0 - dxmin, x1 - dxmin, x1 + dxmax, x0 + dxmax], axis=1)      # [n, 4]
    vy = np.stack([y0 + dymax, y1 + dymax, y1 - dymin, y0 - dymin], axis=1)
    nseg = len(x0)
    e = _edge_records(vx.reshape(-1), vy.reshape(-1), np.roll(vx, -1, axis=1).reshape(-1), np.roll(vy, -1, axis=1).reshape(-1))
    e = e.reshape(nseg, 4, REC)
    head = np.zeros((nseg, 1, REC), dtype=np.int32)
    head[:, 0, 0] = QUAD
    head[:, 0, 1] = np.maximum(vy.min(axis=1), 0)                 # polygon_generic clamps the scan range to [0, ysize]
    head[:, 0, 2] = np.minimum(vy.max(axis=1), s)
    quads = np.concatenate([head, e], axis=1)                     # [n, 5, 8]
    for k in range(nseg):
        if zero[k]:
            pt = np.zeros((1, REC), dtype=np.int32)
            pt[0, :3] = (POINT, x0[k], y0[k])
            out.append(pt)
        else:
            out.append(quads[k])
    return out


def segment_records(path, width):
    """Records of ``ImageDraw.line(path, width=width)`` with the quad geometry left to the device: one SEG per segment,
    carrying hypot(dx, dy) as computed by the host's libm (the one input of Pillow's quad that is not exact arithmetic)."""
    p = np.asarray(path, dtype=np.int32)
    n = len(p) - 1
    rec = np.zeros((n, REC), dtype=np.int32)
    rec[:, 0] = SEG
    rec[:, 1:3], rec[:, 3:5] = p[:-1], p[1:]
    rec[:, 5] = width
    d = (p[1:] - p[:-1]).astype(np.float64)
    rec[:, 6:8] = np.hypot(d[:, 0], d[:, 1]).view(np.int32).reshape(n, 2)          # little endian: lo, hi
    return rec


def brush_records(max_tries, s, min_num_vertex=4, max_num_vertex=18, mean_angle=2 * math.pi / 5, angle_range=2 * math.pi / 15,
                  min_width=12, max_width=48):
    """The draws of ``RandomBrush`` (ds_ffhq.py:145-197) in the reference's order -> (records [n,8], flip0, flip1)."""
    rng = np.random
    mean_radius = math.sqrt(s * s + s * s) / 8
    recs = []
    for _ in range(rng.randint(max_tries)):
        n_vertex = rng.randint(min_num_vertex, max_num_vertex)
        lo = mean_angle - rng.uniform(0, angle_range)
        hi = mean_angle + rng.uniform(0, angle_range)
        ang = rng.uniform(lo, hi, size=n_vertex)                  # same stream as n_vertex scalar draws
        ang[0::2] = 2 * math.pi - ang[0::2]
        path = [(int(rng.randint(0, s)), int(rng.randint(0, s)))]
        steps = np.clip(rng.normal(loc=mean_radius, scale=mean_radius // 2, size=n_vertex), 0, 2 * mean_radius)
        for a, st in zip(ang.tolist(), steps.tolist()):
            px = min(max(path[-1][0] + st * math.cos(a), 0), s)
            py = min(max(path[-1][1] + st * math.sin(a), 0), s)
            path.append((int(px), int(py)))
        thick = int(rng.uniform(min_width, max_width))
        recs.append(segment_records(path, thick))
        discs = np.zeros((len(path), REC), dtype=np.int32)
        discs[:, 0] = DISC
        discs[:, 1:3] = np.asarray(path, dtype=np.int32)
        discs[:, 3] = thick // 2
        recs.append(discs)
        rng.random()                                              # two flip decisions the reference draws and discards
        rng.random()
    flip0 = bool(rng.random() > 0.5)
    flip1 = bool(rng.random() > 0.5)
    return recs, flip0, flip1


def mask_attempt_records(s, hole_range=(0, 1)):
    """One pass of the ``while True`` body of ``RandomMask`` (ds_ffhq.py:199-217) -> (records [n,8] int32, flip0, flip1)."""
    rng = np.random
    coef = min(hole_range[0] + hole_range[1], 1.0)
    recs = []
    for max_tries, max_size in ((int(10 * coef), s // 2), (int(5 * coef), s)):
        for _ in range(rng.randint(max_tries)):
            w, h = rng.randint(max_size), rng.randint(max_size)
            x, y = rng.randint(-(w // 2), s - w + w // 2), rng.randint(-(h // 2), s - h + h // 2)
            x0, x1, y0, y1 = max(x, 0), min(x + w, s) - 1, max(y, 0), min(y + h, s) - 1
            if x0 <= x1 and y0 <= y1:
                r = np.zeros((1, REC), dtype=np.int32)
                r[0, :5] = (RECT, x0, x1, y0, y1)
                recs.append(r)
    brush, f0, f1 = brush_records(int(20 * coef), s)
    recs.extend(brush)
    if recs:
        return np.concatenate(recs, axis=0), f0, f1
    return np.zeros((0, REC), dtype=np.int32), f0, f1


_disc_table = None


def disc_span_table():
    """[MAX_HALF+1, 2*MAX_HALF+1, 2] int32: row j of the filled ellipse with bounding box (c-h, c-h, c+h, c+h) covers columns
    c-h+l .. c-h+r (l > r: empty row).  Read from Pillow -- the reference's rasteriser is the specification."""
    global _disc_table
    if _disc_table is None:
        from PIL import Image, ImageDraw
        t = np.zeros((MAX_HALF + 1, 2 * MAX_HALF + 1, 2), dtype=np.int32)
        t[:, :, 0] = 1
        for h in range(1, MAX_HALF + 1):
            c = Image.new('L', (2 * h + 9, 2 * h + 9), 0)
            ImageDraw.Draw(c).ellipse((4, 4, 4 + 2 * h, 4 + 2 * h), fill=1)
            a = np.asarray(c)
            for j in range(2 * h + 1):
                xs = np.nonzero(a[4 + j])[0]
                if len(xs):
                    t[h, j] = (int(xs[0]) - 4, int(xs[-1]) - 4)
        _disc_table = t
    return _disc_table


def rasterize(records, offsets, flips, s, device='cuda', boxes=None):
    """records [total,8] int32, offsets [B+1], flips [B,2] (host arrays) -> (mask float32 [B,1,s,s] with 1 = keep / 0 = hole,
    hole counts int32 [B]) on ``device``: one H2D copy of the primitive lists, one kernel.  ``boxes`` [B,2] = content (h', w') per
    mask or None: keep is written at x >= w' or y >= h' (FreeFormMaskFormatter of ds_openimages.py:148-166); the hole counts are
    those of the whole mask, before that fill."""
    if s < 32 or s > 1024 or s % 32 != 0:
        raise _lib.ShgError('mask rasteriser: s must be a multiple of 32 in [32, 1024]')
    if records.shape[0] and int(records[records[:, 0] == DISC, 3].max(initial=0)) > MAX_HALF:
        raise _lib.ShgError('mask rasteriser: disc radius beyond the span table')
    dev = torch.device(device)
    b = len(offsets) - 1
    # ONE H2D copy of the primitive lists, from pinned memory: a pageable source of this size (~0.5 MB) takes the runtime's
    # pin-in-place path, which was measured to stall the host for two batches of device work every fourth batch of the evaluation
    # loop (37 ms; MEASUREMENTS.md, round 6).  torch's caching host allocator keeps the block alive until the copy has run.
    rec_h = np.ascontiguousarray(records.reshape(-1), dtype=np.int32) if records.shape[0] else np.zeros(REC, np.int32)
    off_h = np.asarray(offsets, dtype=np.int32)
    flip_h = np.asarray(flips, dtype=np.int32).reshape(-1)
    box_h = np.zeros(0, np.int32) if boxes is None else np.asarray(boxes, dtype=np.int32).reshape(-1)
    if boxes is not None and box_h.size != 2 * b:
        raise _lib.ShgError(f'mask rasteriser: boxes must be [{b}, 2] (got {box_h.size} values)')
    n_rec, n_off, n_flip, n_box = rec_h.size, off_h.size, flip_h.size, box_h.size
    o_off = (n_rec + 3) // 4 * 4                         # 16-byte aligned sections
    o_flip = o_off + (n_off + 3) // 4 * 4
    o_box = o_flip + (n_flip + 3) // 4 * 4
    stage = torch.empty(o_box + n_box, dtype=torch.int32, pin_memory=(dev.type == 'cuda'))
    sv = stage.numpy()
    sv[:n_rec], sv[o_off:o_off + n_off], sv[o_flip:o_flip + n_flip], sv[o_box:o_box + n_box] = rec_h, off_h, flip_h, box_h
    stage_d = stage.to(dev, non_blocking=True)
    rec_d, off_d, flip_d = stage_d[:n_rec], stage_d[o_off:o_off + n_off], stage_d[o_flip:o_flip + n_flip]
    tab_d = _table_on(dev)
    mask = torch.empty((b, 1, s, s), dtype=torch.float32, device=dev)
    holes = torch.zeros((b,), dtype=torch.int32, device=dev)
    L = kernels._Launch()
    for t, nm in ((rec_d, 'records'), (off_d, 'offsets'), (flip_d, 'flips'), (tab_d, 'table'), (holes, 'holes')):
        L.req(t, nm, dtype=torch.int32)
    L.req(mask, 'mask')
    lib = _lib.get_lib()
    with L:
        if boxes is None:
            check(lib.shg_mask_raster_f32(kernels._ptr(rec_d), kernels._ptr(off_d), kernels._ptr(flip_d), kernels._ptr(tab_d), MAX_HALF,
                                          kernels._ptr(mask), kernels._ptr(holes), b, s, L.stream()), 'mask_raster')
        else:
            box_d = stage_d[o_box:o_box + n_box]
            check(lib.shg_mask_raster_box_f32(kernels._ptr(rec_d), kernels._ptr(off_d), kernels._ptr(flip_d), kernels._ptr(tab_d), MAX_HALF,
                                              kernels._ptr(box_d), kernels._ptr(mask), kernels._ptr(holes), b, s, L.stream()), 'mask_raster')
    return mask, holes


_tables = {}


def _table_on(dev):
    key = str(dev)
    if key not in _tables:
        _tables[key] = torch.from_numpy(disc_span_table().reshape(-1).copy()).to(dev)
    return _tables[key]


def random_masks(n, s, hole_range=(0, 1), device='cuda', batch=64, boxes=None):
    """``n`` masks of ``RandomMask(s, hole_range)`` drawn from numpy's global RNG, rasterised on ``device``:
    float32 [n,1,s,s].  Same masks (and same final RNG state) as n sequential calls of the reference function.  ``boxes`` [n,2] =
    content (h', w') of mask i or None: keep is then written at x >= w' or y >= h' after the draw (the box fill of OpenImages'
    ``FreeFormMaskFormatter``); the rejection loop sees the hole ratio of the whole mask, as the reference's does."""
    if boxes is not None:
        boxes = np.asarray(boxes, dtype=np.int32).reshape(n, 2)
    out = []
    while len(out) < n:
        want = min(batch, n - len(out))
        states, recs, offs, flips = [], [], [0], []
        for _ in range(want):
            r, f0, f1 = mask_attempt_records(s, hole_range)
            states.append(np.random.get_state())
            recs.append(r)
            offs.append(offs[-1] + len(r))
            flips.append((int(f0), int(f1)))
        bx = None if boxes is None else boxes[len(out):len(out) + want]
        mask, holes = rasterize(np.concatenate(recs, axis=0) if offs[-1] else np.zeros((0, REC), np.int32), offs, flips, s, device, bx)
        ratio = holes.cpu().numpy().astype(np.float64) / float(s * s)        # the one synchronisation per batch
        ok = ~((ratio <= hole_range[0]) | (ratio >= hole_range[1])) if hole_range is not None else np.ones(want, bool)
        if ok.all():
            out.extend(mask[k] for k in range(want))
            continue
        bad = int(np.argmin(ok))                       # first rejected attempt: everything after it was drawn from a wrong state
        out.extend(mask[k] for k in range(bad))
        np.random.set_state(states[bad])               # the reference loops: the next attempt continues from here
    return torch.stack(out[:n]) if out else torch.empty((0, 1, s, s), device=device)


# ------------------------------------------------------------------------------------------------
# LaMa thin / medium / thick masks (lib/data_factory/lama_mask_utils.py, LamaMaskFormatter of ds_ffhq.py:352-381)
# ------------------------------------------------------------------------------------------------
# The reference draws these with ``cv2.line(mask, p0, p1, 1.0, brush_w)``: OpenCV's ThickLine is the specification -- a convex quad
# in 16.16 fixed point (FillConvexPoly: an outline walk, Line2 behind clipLine, and a two-walker scan), and a filled midpoint circle
# at each end.  The split is the freeform masks': the host makes the draws in the reference's order and emits integer records, the
# device (csrc/mask_lama.hip, ``shg_mask_lama_f32``) rasterises.  There is no rejection loop, so a batch is one H2D copy and one
# launch with no synchronisation.  NOT CHECKED AGAINST cv2: the rasteriser is written down from OpenCV's algorithm and pinned on
# that restatement (tests/lama_cv_ref.py); the draws are pinned on the reference's own generator (tests/golden/lama_masks.npz).

LAMA_RECT, LAMA_LINE = 0, 1               # RECT (0, x0, x1, y0, y1): columns x0 <= x < x1, rows y0 <= y < y1
#                                           LINE (1, x0, y0, x1, y1, t, dpx, dpy): dp = the 16.16 quad offset, filled in by lama_quad_offsets
LAMA_MAX_T = 1023                         # thickness served by the circle table: radius (t + 1) >> 1 <= 512
_XS, _ONE, _HALF = 16, 1 << 16, 1 << 15


def _irr(min_times, max_times, max_width, max_len, max_angle=4):
    return dict(min_times=min_times, max_times=max_times, max_width=max_width, max_angle=max_angle, max_len=max_len)


def _box(margin, bbox_min_size, bbox_max_size, min_times, max_times):
    return dict(margin=margin, bbox_min_size=bbox_min_size, bbox_max_size=bbox_max_size, max_times=max_times, min_times=min_times)


LAMA_SETTINGS = {
    ('thin', 256): dict(irregular_proba=1, irregular_kwargs=_irr(4, 50, 10, 40), box_proba=0, segm_proba=0, squares_proba=0),
    ('medium', 256): dict(irregular_proba=1, irregular_kwargs=_irr(4, 5, 50, 100), box_proba=0.3, box_kwargs=_box(0, 10, 50, 1, 5),
                          segm_proba=0, squares_proba=0),
    ('thick', 256): dict(irregular_proba=1, irregular_kwargs=_irr(1, 5, 100, 200), box_proba=0.3, box_kwargs=_box(10, 30, 150, 1, 3),
                         segm_proba=0, squares_proba=0),
    ('thin', 512): dict(irregular_proba=1, irregular_kwargs=_irr(4, 70, 20, 100), box_proba=0, segm_proba=0, squares_proba=0),
    ('medium', 512): dict(irregular_proba=1, irregular_kwargs=_irr(4, 10, 100, 200), box_proba=0.3, box_kwargs=_box(0, 30, 150, 1, 5),
                          segm_proba=0, squares_proba=0),
    ('thick', 512): dict(irregular_proba=1, irregular_kwargs=_irr(1, 5, 250, 450), box_proba=0.3, box_kwargs=_box(10, 30, 300, 1, 4),
                         segm_proba=0, squares_proba=0),
}
LAMA_KINDS = ('lama_thin', 'lama_medium', 'lama_thick')     # the ``mask_kind`` values of the datasets, DeviceFeeder and EvalLoop


def lama_setting(kind, s):
    """'thin' | 'medium' | 'thick' (or the ``mask_kind`` spelling 'lama_thin' ...) at 256 | 512 -> its setting; anything else is refused."""
    k = kind[5:] if isinstance(kind, str) and kind.startswith('lama_') else kind
    if (k, s) not in LAMA_SETTINGS:
        raise _lib.ShgError(f'LaMa masks: no setting for type {kind!r} at resolution {s!r} (thin / medium / thick at 256 / 512)')
    return LAMA_SETTINGS[(k, s)]


_REFUSED = ('segm', 'squares', 'superres', 'outpainting', 'invert')
_lama_trig = {}


def _trig(max_angle):
    """sin / cos of the 2 * max_angle angles a stroke can take, [parity][k], computed as the reference computes them (numpy)."""
    if max_angle not in _lama_trig:
        tab = []
        for even in (False, True):
            ang = [(2 * 3.1415926 - (0.01 + k)) if even else (0.01 + k) for k in range(max_angle)]
            tab.append([(float(np.sin(a)), float(np.cos(a))) for a in ang])
        _lama_trig[max_angle] = tab
    return _lama_trig[max_angle]


def _trunc_clip(f, hi):
    """``np.clip(f.astype(np.int32), 0, hi)`` of a double well inside the int32 range."""
    return min(max(int(f), 0), hi)


def lama_mask_records(s, setting):
    """One call of ``MixedMaskGenerator(**setting).__call__`` on an s x s image, drawn from numpy's global RNG in the reference's order
    (lama_mask_utils.py:365-368, :79-105, :129-140; the ramps at coef = 1) -> int32 records [n, 8]: LINE (1, x0, y0, x1, y1, t, 0, 0)
    per ``cv2.line`` call, RECT (0, x0, x1, y0, y1) per box.  Options the reference's generator would take another path for are refused."""
    for name in _REFUSED:
        if setting.get(name + '_proba', 0) > 0:
            raise _lib.ShgError(f'LaMa masks: the {name} option is not served')
    if any(k not in ('irregular_proba', 'irregular_kwargs', 'box_proba', 'box_kwargs') and not (k[:-6] in _REFUSED and k.endswith('_proba'))
           for k in setting):
        raise _lib.ShgError(f'LaMa masks: unknown options in {sorted(setting)}')
    if set(setting.get('irregular_kwargs') or {}) - {'max_angle', 'max_len', 'max_width', 'min_times', 'max_times'}:
        raise _lib.ShgError('LaMa masks: irregular_kwargs hold an option that is not served (ramp, draw method)')
    if set(setting.get('box_kwargs') or {}) - {'margin', 'bbox_min_size', 'bbox_max_size', 'min_times', 'max_times'}:
        raise _lib.ShgError('LaMa masks: box_kwargs hold an option that is not served (ramp)')
    rng = np.random
    probas, gens = [], []
    if setting.get('irregular_proba', 1 / 3) > 0:
        probas.append(setting.get('irregular_proba', 1 / 3))
        gens.append('irregular')
    if setting.get('box_proba', 1 / 3) > 0:
        probas.append(setting.get('box_proba', 1 / 3))
        gens.append('box')
    if not gens:
        raise _lib.ShgError('LaMa masks: the setting enables no generator')
    p = np.array(probas, dtype='float32')
    p /= p.sum()
    gen = gens[rng.choice(len(p), p=p)]                       # consumes a draw even when there is one generator
    out = []
    if gen == 'irregular':
        kw = dict(max_angle=4, max_len=60, max_width=20, min_times=0, max_times=10)
        kw.update(setting.get('irregular_kwargs') or {})
        max_len, max_width = int(max(1, kw['max_len'])), int(max(1, kw['max_width']))
        max_times = int(kw['min_times'] + 1 + (kw['max_times'] - kw['min_times']))
        max_angle, trig = kw['max_angle'], _trig(kw['max_angle'])
        ri = rng.randint
        for i in range(ri(kw['min_times'], max_times + 1)):
            x, y = ri(s), ri(s)
            tab = trig[i % 2 == 0]
            for _ in range(1 + ri(5)):
                sn, cs = tab[ri(max_angle)]
                length = 10 + ri(max_len)
                t = 5 + ri(max_width)
                ex, ey = _trunc_clip(x + length * sn, s), _trunc_clip(y + length * cs, s)
                out.append((LAMA_LINE, x, y, ex, ey, t, 0, 0))
                x, y = ex, ey
    else:
        kw = dict(margin=10, bbox_min_size=30, bbox_max_size=100, min_times=0, max_times=3)
        kw.update(setting.get('box_kwargs') or {})
        margin, lo = kw['margin'], kw['bbox_min_size']
        hi = int(lo + 1 + (kw['bbox_max_size'] - lo))
        max_times = int(kw['min_times'] + (kw['max_times'] - kw['min_times']))
        hi = min(hi, s - margin * 2, s - margin * 2)
        for _ in range(rng.randint(kw['min_times'], max_times + 1)):
            bw, bh = rng.randint(lo, hi), rng.randint(lo, hi)
            x, y = rng.randint(margin, s - margin - bw + 1), rng.randint(margin, s - margin - bh + 1)
            out.append((LAMA_RECT, x, x + bw, y, y + bh, 0, 0, 0))
    if any(r[0] == LAMA_LINE and r[5] <= 1 for r in out):
        raise _lib.ShgError('LaMa masks: thickness <= 1 takes another rasteriser (a plain Line), which is not served')
    return np.asarray(out, dtype=np.int32).reshape(-1, REC)


def lama_check_records(records, s):
    """The host-side refusals shared by the device and the host rasteriser -> records as int32 [n, 8]."""
    if s < 32 or s > 512 or s % 32 != 0:
        raise _lib.ShgError(f'LaMa masks: s must be a multiple of 32 in [32, 512] (got {s})')
    rec = np.asarray(records, dtype=np.int32).reshape(-1, REC)
    if rec.shape[0]:
        ty = rec[:, 0]
        if ((ty != LAMA_RECT) & (ty != LAMA_LINE)).any():
            raise _lib.ShgError('LaMa masks: unknown record type')
        ln = rec[ty == LAMA_LINE]
        if ln.shape[0] and (ln[:, 5].min() < 2 or ln[:, 5].max() > LAMA_MAX_T):
            raise _lib.ShgError(f'LaMa masks: thickness must lie in [2, {LAMA_MAX_T}]')
        if np.abs(rec[:, 1:5]).max() > 2048:
            raise _lib.ShgError('LaMa masks: coordinates beyond +-2048')
    return rec


def lama_quad_offsets(records):
    """Fill dp = (cvRound(dy * r), cvRound(dx * r)) of every LINE record (ThickLine; r = half the thickness in 16.16 over the segment's
    length): the one step that is not exact integer arithmetic -- the host's sqrt and round-half-even, shipped as integers.  A
    zero-length segment keeps dp = 0 (it is its two circles)."""
    rec = np.array(records, dtype=np.int32).reshape(-1, REC)
    ln = np.nonzero(rec[:, 0] == LAMA_LINE)[0] if rec.shape[0] else np.zeros(0, np.int64)
    if len(ln):
        q = rec[ln].astype(np.int64)
        dx = ((q[:, 1] - q[:, 3]) << _XS) / 65536.0
        dy = ((q[:, 4] - q[:, 2]) << _XS) / 65536.0
        r = dx * dx + dy * dy
        t = q[:, 5]
        ok = np.abs(r) > np.finfo(np.float64).eps
        num = (t << (_XS - 1)) + (t & 1) * _ONE * 0.5
        r = num / np.sqrt(np.where(ok, r, 1.0))
        rec[ln, 6] = np.where(ok, np.rint(dy * r), 0).astype(np.int32)
        rec[ln, 7] = np.where(ok, np.rint(dx * r), 0).astype(np.int32)
    return rec


_lama_circle = None


def lama_circle_table():
    """int32 [513, 513]: row j (|offset| from the centre row) of the filled ``Circle`` of radius r covers columns cx - hw .. cx + hw with
    hw = table[r, j]; -1 = no row.  From the integer midpoint walk itself (the union of its spans per row); nothing is read from cv2."""
    global _lama_circle
    if _lama_circle is None:
        rmax = (LAMA_MAX_T + 1) >> 1
        tab = np.full((rmax + 1, rmax + 1), -1, dtype=np.int32)
        for r in range(rmax + 1):
            row = tab[r]
            err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
            while dx >= dy:
                if dx > row[dy]:
                    row[dy] = dx
                if dy > row[dx]:
                    row[dx] = dy
                dy += 1
                err += plus
                plus += 2
                if err > 0:
                    err -= minus
                    dx -= 1
                    minus -= 2
        _lama_circle = tab
    return _lama_circle


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _lama_clip(w, h, x1, y1, x2, y2):
    """OpenCV's ``clipLine`` on Python ints; the product and the quotient of its double expression are rounded separately."""
    right, bottom = w - 1, h - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1, c1 = a, 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2, c2 = a, 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def _lama_points(img, px, py):
    ok = (px >= 0) & (px < img.shape[1]) & (py >= 0) & (py < img.shape[0])
    img[py[ok], px[ok]] = 1


def _lama_outline(img, a, b):
    """``Line2`` with the steps of its walk taken at once: pixel k is (x1 + k, (y1 + k * y_step) >> 16), exact in integers."""
    s = img.shape[0]
    ok, x1, y1, x2, y2 = _lama_clip(s << _XS, s << _XS, a[0], a[1], b[0], b[1])
    if not ok:
        return
    dx, dy = x2 - x1, y2 - y1
    xmajor = abs(dx) > abs(dy)
    if not xmajor:                                   # the y-major walk is the x-major one with the axes exchanged
        x1, y1, x2, y2, dx, dy = y1, x1, y2, x2, dy, dx
    if dx < 0:
        x1, y1, x2, y2, dy = x2, y2, x1, y1, -dy
    step = _tdiv(dy << _XS, abs(dx) | 1)
    k = np.arange(((x2 - x1) >> _XS) + 1, dtype=np.int64)
    pu = np.concatenate([[(x2 + _HALF) >> _XS], ((x1 + _HALF) >> _XS) + k])
    pv = np.concatenate([[(y2 + _HALF) >> _XS], (y1 + _HALF + k * step) >> _XS])
    if xmajor:
        _lama_points(img, pu, pv)
    else:
        _lama_points(img, pv, pu)


def _lama_quad(img, v):
    """``FillConvexPoly`` of four 16.16 vertices.  The two edge walkers change state only at the rows where an edge ends, and between
    those rows x is xs + (y - y_set) * dx in exact integers: the walk is made event by event, the rows of a piece at once -- the
    form the device kernel uses, one lane per row."""
    s = img.shape[0]
    for i, j in ((3, 0), (0, 1), (1, 2), (2, 3)):
        _lama_outline(img, v[i], v[j])
    vx, vy = [p[0] for p in v], [p[1] for p in v]
    imin = vy.index(min(vy))
    xmin, xmax = (min(vx) + _HALF) >> _XS, (max(vx) + _HALF) >> _XS
    ymin, ymax = (min(vy) + _HALF) >> _XS, (max(vy) + _HALF) >> _XS
    if xmax < 0 or ymax < 0 or xmin >= s or ymin >= s:
        return
    ymax = min(ymax, s - 1)
    idx, di, xs, dx, ye, ys = [imin, imin], (1, 3), [-_ONE, -_ONE], [0, 0], [ymin, ymin], [ymin, ymin]
    edges, yc = 4, ymin
    while yc <= ymax:
        for i in range(2):
            if yc >= ye[i]:
                idx0 = idx[i]
                k = (idx0 + di[i]) & 3
                while True:
                    edges -= 1
                    if edges < 0:
                        break
                    ty = (vy[k] + _HALF) >> _XS
                    if ty > yc:
                        xs[i], ys[i], ye[i], idx[i] = vx[idx0], yc, ty, k
                        dx[i] = _tdiv((vx[k] - vx[idx0]) * 2 + (ty - yc), 2 * (ty - yc))
                        break
                    idx0 = k
                    k = (k + di[i]) & 3
        if edges < 0:
            return
        ynext = min(ye[0], ye[1])
        lo, hi = max(yc, 0), min(ynext - 1, ymax)
        if lo <= hi:
            rows = np.arange(lo, hi + 1, dtype=np.int64)
            xa, xb = xs[0] + (rows - ys[0]) * dx[0], xs[1] + (rows - ys[1]) * dx[1]
            x1, x2 = (np.minimum(xa, xb) + _HALF) >> _XS, (np.maximum(xa, xb) + _HALF) >> _XS
            for y, l, r in zip(rows.tolist(), x1.tolist(), x2.tolist()):
                if r >= 0 and l < s:
                    img[y, max(l, 0):min(r, s - 1) + 1] = 1
        yc = ynext


def _lama_disc(img, cx, cy, r):
    s = img.shape[0]
    hw = lama_circle_table()[r]
    for j in range(-r, r + 1):
        y, h = cy + j, int(hw[abs(j)])
        if 0 <= y < s and h >= 0:
            l, rr = max(cx - h, 0), min(cx + h, s - 1)
            if l <= rr:
                img[y, l:rr + 1] = 1


def lama_draw_host(records, s):
    """Painted pixels (uint8 [s,s], 1 = hole) of one mask's records on the host: the device kernel's arithmetic in numpy."""
    rec = lama_quad_offsets(lama_check_records(records, s))
    img = np.zeros((s, s), np.uint8)
    for ty, a, b, c, d, t, dpx, dpy in rec.tolist():
        if ty == LAMA_RECT:
            img[max(c, 0):max(d, 0), max(a, 0):max(b, 0)] = 1
            continue
        p0, p1 = (a << _XS, b << _XS), (c << _XS, d << _XS)
        if p0 != p1:
            _lama_quad(img, [(p0[0] + dpx, p0[1] + dpy), (p0[0] - dpx, p0[1] - dpy), (p1[0] - dpx, p1[1] - dpy), (p1[0] + dpx, p1[1] + dpy)])
        r = ((t << (_XS - 1)) + _HALF) >> _XS
        _lama_disc(img, a, b, r)
        _lama_disc(img, c, d, r)
    return img


_lama_tables = {}


def lama_rasterize(records, offsets, s, device='cuda'):
    """records [total, 8] int32 (LINE / RECT, ``lama_mask_records``), offsets [B+1] (host arrays) -> (mask float32 [B,1,s,s] with 1 = keep /
    0 = hole, hole counts int32 [B]) on ``device``: every argument is checked on the host, then ONE pinned H2D copy of the records and
    ONE launch on the current stream; nothing waits for the device."""
    rec = lama_quad_offsets(lama_check_records(records, s))
    off_h = np.asarray(offsets, dtype=np.int32).reshape(-1)
    b = off_h.size - 1
    if b < 1 or off_h[0] != 0 or off_h[-1] != rec.shape[0] or (np.diff(off_h) < 0).any():
        raise _lib.ShgError('LaMa masks: offsets must rise from 0 to the number of records, one mask at least')
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _lib.ShgError('LaMa masks: the rasteriser runs on a HIP (cuda) device; data.LamaMask is the host path')
    n_rec = max(rec.size, REC)
    o_off = (n_rec + 3) // 4 * 4
    stage = torch.zeros(o_off + off_h.size, dtype=torch.int32, pin_memory=True)       # pinned: see ``rasterize``
    sv = stage.numpy()
    sv[:rec.size], sv[o_off:] = rec.reshape(-1), off_h
    stage_d = stage.to(dev, non_blocking=True)
    rec_d, off_d = stage_d[:n_rec], stage_d[o_off:]
    key = str(dev)
    if key not in _lama_tables:
        _lama_tables[key] = torch.from_numpy(lama_circle_table().reshape(-1).copy()).to(dev)
    tab_d = _lama_tables[key]
    mask = torch.empty((b, 1, s, s), dtype=torch.float32, device=dev)
    holes = torch.empty((b,), dtype=torch.int32, device=dev)
    L = kernels._Launch()
    for t, nm in ((rec_d, 'records'), (off_d, 'offsets'), (tab_d, 'table'), (holes, 'holes')):
        L.req(t, nm, dtype=torch.int32)
    L.req(mask, 'mask')
    with L:
        # the C entry point checks every record on the host, from the staging buffer itself, before it launches
        check(_lib.get_lib().shg_mask_lama_f32(stage.data_ptr(), stage.data_ptr() + 4 * o_off, kernels._ptr(rec_d), kernels._ptr(off_d),
                                               kernels._ptr(tab_d), (LAMA_MAX_T + 1) >> 1, kernels._ptr(mask), kernels._ptr(holes), b,
                                               int(off_h[-1]), s, L.stream()), 'mask_lama')
    return mask, holes


def lama_masks(n, s, kind, device='cuda'):
    """``n`` masks of ``LamaMaskFormatter(resolution=s, type=kind)`` (``1 - mask``: 1 = keep, 0 = hole) drawn from numpy's global RNG and
    rasterised on ``device`` -> (float32 [n,1,s,s], hole counts int32 [n], both on the device).  Same masks and same final RNG state as
    n sequential calls of the reference's generator; one H2D copy, one launch, no synchronisation."""
    setting = lama_setting(kind, s)
    if n < 1:
        raise _lib.ShgError('LaMa masks: n must be >= 1')
    recs, offs = [], [0]
    for _ in range(n):
        r = lama_mask_records(s, setting)
        recs.append(r)
        offs.append(offs[-1] + len(r))
    return lama_rasterize(np.concatenate(recs, axis=0), offs, s, device)
