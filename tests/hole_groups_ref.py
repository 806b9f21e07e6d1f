"""Yardstick of the hole groups (sh-gan_amd/inpaint.py ``label_holes`` / ``owner_plane`` on csrc/hole_label.hip):
pure numpy restatements and the cases the device is held to, bit for bit.  Nothing here is shipped.

Conventions as the module's: mask != 0 known, 0 hole; r = feather + 1; D = the pixels within Chebyshev distance r of a hole pixel of the
same image; a group is an 8-connected component of D, its root the smallest y w + x over its pixels."""
import numpy as np


def dilate(hole, r):
    """bool [h, w] -> D: a hole within r along the row, then within r along the column (clipped to the image)."""
    h, w = hole.shape
    row = hole.copy()
    for d in range(1, min(r, w - 1) + 1):
        row[:, d:] |= hole[:, :w - d]
        row[:, :w - d] |= hole[:, d:]
    out = row.copy()
    for d in range(1, min(r, h - 1) + 1):
        out[d:] |= row[:h - d]
        out[:h - d] |= row[d:]
    return out


def groups_reference(mask, feather, image=0):
    """-> (labels int32 [h, w]: the root inside D, -1 elsewhere; components int64 [C, 7] = (image, root, ya, yb, xa, xb, hole pixels)
    sorted by root).  A flood over an explicit stack; pixels are visited in row-major order, so the pixel a flood starts from is the
    smallest of its component: the root."""
    mask = np.asarray(mask)
    h, w = mask.shape
    hole = mask == 0
    D = dilate(hole, int(feather) + 1)
    labels = np.full((h, w), -1, np.int32)
    comps = []
    for start in np.flatnonzero(D.reshape(-1)):
        y, x = divmod(int(start), w)
        if labels[y, x] >= 0:
            continue
        labels[y, x] = start
        stack = [(y, x)]
        ya, yb, xa, xb, cnt = h, 0, w, 0, 0
        while stack:
            y, x = stack.pop()
            if hole[y, x]:
                ya, yb, xa, xb, cnt = min(ya, y), max(yb, y + 1), min(xa, x), max(xb, x + 1), cnt + 1
            for ny in range(max(y - 1, 0), min(y + 2, h)):
                for nx in range(max(x - 1, 0), min(x + 2, w)):
                    if D[ny, nx] and labels[ny, nx] < 0:
                        labels[ny, nx] = start
                        stack.append((ny, nx))
        comps.append((image, int(start), ya, yb, xa, xb, cnt))
    return labels, np.array(comps, np.int64).reshape(-1, 7)


def pack_reference(masks, feather):
    """A list of masks -> (labels int32 [sum h w] in packed-mask layout, components int64 [C, 7] sorted by (image, root))."""
    labs, comps = zip(*[groups_reference(m, feather, i) for i, m in enumerate(masks)])
    return np.concatenate([l.reshape(-1) for l in labs]), np.concatenate(comps)


def owner_reference(mask, labels, keys):
    """keys: {root: key} -> uint8 [h, w]: 0 at known pixels, the key of its group's root at a hole pixel (0 for a root keys lacks)."""
    mask, labels = np.asarray(mask), np.asarray(labels)
    out = np.zeros(mask.shape, np.uint8)
    for root, key in keys.items():
        out[(labels == root) & (mask == 0)] = key
    return out


def group_masks(mask, feather):
    """-> [(root, mask known everywhere but that group's holes)] in order of increasing root."""
    labels, comps = groups_reference(mask, feather)
    return [(int(c[1]), np.where((labels == c[1]) & (np.asarray(mask) == 0), 0, 1).astype(np.uint8)) for c in comps]


# numpy stand-ins of label_holes + fetch_components / owner_plane for ``Inpainter(label_fn=, owner_fn=)``

def label_fn(packed_mask, shapes, feather):
    pm = np.asarray(packed_mask.cpu().numpy() if hasattr(packed_mask, 'cpu') else packed_mask)
    return pack_reference([pm[moff:moff + h * w].reshape(h, w) for h, w, _, moff in np.asarray(shapes)], feather)[1]


def owner_fn(packed_mask, shapes, table, feather):
    import torch
    pm = np.asarray(packed_mask.cpu().numpy() if hasattr(packed_mask, 'cpu') else packed_mask)
    out = np.zeros_like(pm)
    for i, (h, w, _, moff) in enumerate(np.asarray(shapes)):
        m = pm[moff:moff + h * w].reshape(h, w)
        keys = {int(r): int(k) for im, r, k in np.asarray(table).reshape(-1, 3) if im == i}
        out[moff:moff + h * w] = owner_reference(m, groups_reference(m, feather)[0], keys).reshape(-1)
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------

def _ones(h, w):
    return np.ones((h, w), np.uint8)


def _with(h, w, pixels=(), boxes=()):
    m = _ones(h, w)
    for y, x in pixels:
        m[y, x] = 0
    for ya, yb, xa, xb in boxes:
        m[ya:yb, xa:xb] = 0
    return m


def comb(h, w, period):
    """A spine along row 0 with one-pixel teeth every ``period`` columns running down the whole image."""
    m = _ones(h, w)
    m[0, :] = 0
    m[:, ::period] = 0
    return m


def spiral(h, w, pitch):
    """A one-pixel rectangular spiral whose arms lie ``pitch`` apart: one component whose label chain winds through the whole image."""
    m = _ones(h, w)
    y0, y1, x0, x1 = 0, h - 1, 0, w - 1
    m[y0, x0:x1 + 1] = 0                                             # top, rightwards
    while y1 - y0 >= pitch and x1 - x0 >= pitch:
        m[y0:y1 + 1, x1] = 0                                         # right side, down
        m[y1, x0:x1 + 1] = 0                                         # bottom, leftwards
        y0 += pitch
        if y1 - y0 < pitch:
            break
        m[y0:y1 + 1, x0] = 0                                         # left side, up to the next top
        x1 -= pitch
        if x1 - x0 < pitch:
            break
        m[y0, x0:x1 + 1] = 0                                         # the next top
        y1, x0 = y1 - pitch, x0 + pitch
    return m


def gap_cases(T, r):
    """Two single-pixel holes with a gap of 2r (one group) and 2r + 1 (two groups) known pixels between them, along a row, a column and
    the diagonal, the gap's middle on a tile seam (coordinate T away from a corner) and on the four-tile corner (T, T).  -> [(name, mask,
    groups expected)]."""
    h = w = 2 * T + 3
    out = []
    for gap, want in ((2 * r, 1), (2 * r + 1, 2)):
        a, b = T - gap // 2 - 1, T - gap // 2 + gap                   # the two holes' coordinates: b - a - 1 = gap, the seam between
        for where, c in (('seam', T // 2), ('corner', T)):
            out.append((f'row-{where}-gap{gap}', _with(h, w, [(c, a), (c, b)]), want))
            out.append((f'col-{where}-gap{gap}', _with(h, w, [(a, c), (b, c)]), want))
        out.append((f'diag-corner-gap{gap}', _with(h, w, [(a, a), (b, b)]), want))
        out.append((f'anti-corner-gap{gap}', _with(h, w, [(a, b), (b, a)]), want))
    return out


def single_cases(T, r):
    """-> [(name, mask)] of the single-image cases."""
    out = []
    for h, w in ((5, 7), (T, T), (T + 1, T - 1), (2 * T + 3, 3 * T + 1)):
        rng = np.random.RandomState(h * 1000 + w)
        out.append((f'empty-{h}x{w}', _ones(h, w)))
        out.append((f'all-{h}x{w}', np.zeros((h, w), np.uint8)))
        out.append((f'corners-{h}x{w}', _with(h, w, [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)])))
        out.append((f'random-{h}x{w}', (rng.random_sample((h, w)) > 0.004).astype(np.uint8)))
    out += [(n, m) for n, m, _ in gap_cases(T, r)]
    # D touching only diagonally across the four-tile corner: holes whose dilated squares end at (T - 1, T - 1) and begin at (T, T), and
    # the mirrored pair
    h = w = 2 * T + 3
    out.append(('dtouch-diag', _with(h, w, [(T - 1 - r, T - 1 - r), (T + r, T + r)])))
    out.append(('dtouch-anti', _with(h, w, [(T - 1 - r, T + r), (T + r, T - 1 - r)])))
    out.append(('comb', comb(2 * T, 2 * T, 2 * r + 2)))
    out.append(('spiral', spiral(2 * T, 2 * T, 2 * r + 2)))
    # column w - 1 and column 0 of consecutive rows are no neighbours
    out.append(('wrap', _with(T + 1, 2 * r + 4, [(3, 2 * r + 3), (4, 0)])))
    return out


def pack_case(T, r):
    """Five ragged images for one launch: a hole in the last row of image i above a hole in the first row of image i + 1, and the rest."""
    return [_with(9, 11, [(8, 5)]), _with(T + 1, 11, [(0, 5), (T, 10)]), _with(2 * T + 3, T + 5, [(0, 0)], [(T - 2, T + 2, T - 3, T + 4)]),
            spiral(T + 9, T + 2, 2 * r + 2), _with(7, 3 * T + 1, [(3, 0), (3, 3 * T)])]


def random_masks(n, seed=0):
    """n small random masks with sparse holes (a few blobs and single pixels) for the invariant sweeps."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        h, w = rng.randint(12, 48, 2)
        m = _ones(h, w)
        for _ in range(rng.randint(1, 5)):
            y, x = rng.randint(0, h), rng.randint(0, w)
            m[y:y + rng.randint(1, 6), x:x + rng.randint(1, 6)] = 0
        out.append(m)
    return out
