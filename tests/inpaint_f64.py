"""Yardstick of sh-gan_amd/inpaint.py: numpy restatements of the window gather and the feathered paste-back, and the byte rule a device
result is held to.  Nothing here is shipped.

Conventions as the module's: mask != 0 known, 0 hole; images uint8 HWC; a window is (y0, x0, ch, cw).

THE BYTE RULE FOR ``paste_back``.  With the float64 restatement (``paste_reference(..., np.float64)``: float64 tap weights, float64
arithmetic) giving the pre-truncation value t and the byte floor(t), a result under test must
  (a) differ from the float64 byte by at most 1 everywhere,
  (b) equal it wherever A = 0 (nothing is computed there: the byte is the original's),
  (c) equal it wherever t is farther than eps from an integer,
and (d) the pixels (c) leaves out are at most 1 % of the case's window pixels (``CAP``).

    eps = 255 (Kh + Kv + 10) 2^-24 max_y sum_j |wy[y, j]| max_x sum_j |wx[x, j]|          (Kh, Kv: the widths of the case's tap tables)

Derivation (u = 2^-24, the unit roundoff of float32; |fake| <= 1 in the cases the rule is applied to).  The horizontal pass computes
sum_j wx_j f_j with float32 weights (each within u |wx_j| of the float64 weight) in a chain of Kh fused multiply-adds: its error is at
most (Kh + 1) u sum|wx| max|f| to first order (the standard bound of a K-term recursive sum, gamma_K, plus the weights' rounding).  The
vertical pass adds (Kv + 1) u sum|wy| max|mid| of its own and carries the first error multiplied by sum|wy|, and max|mid| <= sum|wx|:
|v32 - v64| <= (Kh + Kv + 2) u sum|wy| sum|wx|.  Then v 127.5, + 127.5, A g, + (F - A) orig and / F are five more roundings of values
of magnitude <= 255 sum|wy| sum|wx| (the blend is a convex combination, so it does not amplify what it is given), and the first-order
terms dropped above are covered by three more units: (Kh + Kv + 10) u, times the scale 255 sum|wy| sum|wx| (127.5 |v| + 127.5 <= 255
sum|wy| sum|wx| since the sums are >= 1).  For an upscale both tables have 5 taps and sum|w| <= 1.25: eps ~ 4.8e-4.  Where t is farther
than eps from an integer no float32 evaluation inside the bound can truncate to another byte; where it is nearer, the byte may be the
neighbouring one, which is (a).  The cap: t is spread over the integers' neighbourhoods with density ~ 2 eps per byte, ~ 3e-3 per pixel
of three channels, so 1 % holds with room while a systematic error (a wrong tap, a shifted row) leaves it at once.  Random cases draw
fake uniformly in [-0.6, 0.6]: g stays inside (0, 255) and nothing clamps onto an exact integer.

Two refinements for a ``fake`` that is not of that kind (a generator with random weights saturates: |fake| reaches 20 and most of the hole
clamps).  The forward error is linear in the data, so eps is multiplied by max(1, max|fake|).  And a byte whose float64 v 127.5 + 127.5
lies at least eps outside [0, 255] is NOT left out of the equality although its t may be an exact integer: the float32 value lies
outside as well, g is exactly 0 or 255 in both precisions, A g + (F - A) orig is an integer below 2^24 and exact in both, and the
quotient by F is either that exact integer or at least 1 / F >= 1 / 33 away from one, where two correctly rounded divisions of the same
rational truncate alike."""
import numpy as np

from shgan_amd import inpaint, resize

CAP = 0.01


# ------------------------------------------------------------------------------------------------
# the planner's properties
# ------------------------------------------------------------------------------------------------

def hole_box(mask):
    hole = np.asarray(mask) == 0
    rows, cols = np.flatnonzero(hole.any(axis=1)), np.flatnonzero(hole.any(axis=0))
    return None if rows.size == 0 else (int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1)


def check_window(mask, window, R, context, feather):
    """The properties ``plan_window`` promises, asserted."""
    H, W = np.asarray(mask).shape
    box = hole_box(mask)
    if box is None:
        assert window is None
        return
    ya, yb, xa, xb = box
    y0, x0, ch, cw = window
    assert all(isinstance(v, int) for v in window)
    assert 0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= H and x0 + cw <= W                      # inside the image
    side = max(yb - ya, xb - xa)
    s = max(R, int(np.ceil((1 + 2 * context) * side)), side + 2 * (feather + 2))
    assert ch == min(s, H) and cw == min(s, W)                                                                # square and >= R where the image allows
    margin = feather + 2
    assert y0 <= max(ya - margin, 0) and y0 + ch >= min(yb + margin, H)                                       # the box + feather + 2 where the image allows
    assert x0 <= max(xa - margin, 0) and x0 + cw >= min(xb + margin, W)
    # centred unless the image's border pushes it
    assert y0 in (0, H - ch) or abs((2 * y0 + ch) - (ya + yb)) <= 1
    assert x0 in (0, W - cw) or abs((2 * x0 + cw) - (xa + xb)) <= 1


# ------------------------------------------------------------------------------------------------
# gather
# ------------------------------------------------------------------------------------------------

def pool_mask_bruteforce(mask_win, R):
    """Output pixel (i, j) is known iff every native pixel of rows [i ch // R, max(ceil((i + 1) ch / R), lo + 1)) x the same columns is."""
    ch, cw = mask_win.shape
    out = np.zeros((R, R), np.float32)
    for i in range(R):
        rlo = i * ch // R
        rhi = max(-(-(i + 1) * ch // R), rlo + 1)
        for j in range(R):
            clo = j * cw // R
            chi = max(-(-(j + 1) * cw // R), clo + 1)
            out[i, j] = float(np.all(mask_win[rlo:rhi, clo:chi] != 0))
    return out


def pool_mask(mask_win, R):
    """The same, separable: a footprint is all known iff no hole lies in it (prefix sums of the hole count)."""
    ch, cw = mask_win.shape
    hole = np.zeros((ch + 1, cw + 1), np.int64)
    hole[1:, 1:] = np.cumsum(np.cumsum(mask_win == 0, axis=0), axis=1)
    i = np.arange(R, dtype=np.int64)
    rlo, clo = i * ch // R, i * cw // R
    rhi, chi = np.maximum(-(-(i + 1) * ch // R), rlo + 1), np.maximum(-(-(i + 1) * cw // R), clo + 1)
    cnt = hole[rhi][:, chi] - hole[rlo][:, chi] - hole[rhi][:, clo] + hole[rlo][:, clo]
    return (cnt == 0).astype(np.float32)


def gather_reference(img, mask, window, R):
    """-> (uint8 [3, R, R], float32 [R, R]): ``resize.resize_reference`` of the cropped array (= Pillow's crop().resize() bytes, which
    tests/test_inpaint_cpu.py checks) and the pooled mask."""
    y0, x0, ch, cw = window
    crop = np.ascontiguousarray(np.asarray(img, np.uint8)[y0:y0 + ch, x0:x0 + cw])
    return resize.resize_reference(crop, R), pool_mask(np.asarray(mask)[y0:y0 + ch, x0:x0 + cw], R)


# ------------------------------------------------------------------------------------------------
# feather
# ------------------------------------------------------------------------------------------------

def feather_bruteforce(mask_win, feather):
    """A = max(0, F - d), d the Chebyshev distance to the nearest hole pixel of the window, F = feather + 1: a loop over pixels."""
    F = feather + 1
    ch, cw = mask_win.shape
    hole = mask_win == 0
    out = np.zeros((ch, cw), np.uint8)
    for y in range(ch):
        for x in range(cw):
            for d in range(F):
                if hole[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1].any():
                    out[y, x] = F - d
                    break
    return out


def feather_reference(mask_win, feather):
    """The same, separable: row distance capped at F, then min over dy of max(|dy|, row distance)."""
    F = feather + 1
    ch, cw = mask_win.shape
    hole = mask_win == 0
    rowd = np.full((ch, cw), F, np.int64)
    for d in range(min(F, cw) - 1, -1, -1):
        near = np.zeros((ch, cw), bool)
        near[:, d:] |= hole[:, :cw - d] if d else hole
        if d:
            near[:, :cw - d] |= hole[:, d:]
        rowd[near] = d
    best = rowd.copy()
    for d in range(1, min(F, ch)):
        up = np.full((ch, cw), F, np.int64)
        up[d:] = rowd[:ch - d]
        dn = np.full((ch, cw), F, np.int64)
        dn[:ch - d] = rowd[d:]
        best = np.minimum(best, np.maximum(d, np.minimum(up, dn)))
    return (F - np.minimum(best, F)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# paste
# ------------------------------------------------------------------------------------------------

def _fma(dtype, a, b, c):
    """a b + c rounded once to ``dtype`` (float32: the product is exact in float64, the sum is rounded to float64 and then to float32)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(dtype)


def _resample_pass(x, bounds, w, axis, dtype):
    """One pass along ``axis`` of x [3, h, w]: per output index the chain acc = fma(w_j, x[first + j], acc) over its taps, from 0."""
    x = np.moveaxis(x, axis, 0)
    first, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    acc = np.zeros((w.shape[0],) + x.shape[1:], dtype)
    tail = (slice(None),) + (None,) * (x.ndim - 1)
    for j in range(w.shape[1]):
        idx = np.minimum(first + j, x.shape[0] - 1)
        wj = np.where(j < n, w[:, j], 0.0).astype(dtype)
        acc = _fma(dtype, np.broadcast_to(wj[tail], acc.shape), x[idx], acc)
    return np.moveaxis(acc, 0, axis)


def resample_reference(fake, ch, cw, dtype):
    """fake [3, R, R] -> [3, ch, cw] in ``dtype``: horizontal pass first, then vertical, the weights of ``inpaint.bicubic_weights``."""
    R = fake.shape[-1]
    bx, wx = inpaint.bicubic_weights(R, cw)
    by, wy = inpaint.bicubic_weights(R, ch)
    mid = _resample_pass(np.asarray(fake).astype(dtype), bx, wx.astype(dtype), 2, dtype)
    return _resample_pass(mid, by, wy.astype(dtype), 1, dtype)


def paste_reference(img, mask, window, fake, feather, dtype=np.float64):
    """One image, one sample -> (result uint8 [h, w, 3], t [ch, cw, 3] the pre-truncation values in ``dtype``, A uint8 [ch, cw], raw
    [ch, cw, 3] = v 127.5 + 127.5 before the clamp)."""
    y0, x0, ch, cw = window
    img = np.asarray(img, np.uint8)
    F = feather + 1
    A = feather_reference(np.asarray(mask)[y0:y0 + ch, x0:x0 + cw], feather)
    v = resample_reference(fake, ch, cw, dtype).transpose(1, 2, 0)
    c = dtype(127.5)
    raw = v * c + c
    g = np.clip(raw, dtype(0), dtype(255))
    a = A[:, :, None].astype(dtype)
    orig = img[y0:y0 + ch, x0:x0 + cw].astype(dtype)
    t = (a * g + (dtype(F) - a) * orig) / dtype(F)
    assert t.dtype == dtype
    out = img.copy()
    out[y0:y0 + ch, x0:x0 + cw] = np.where(A[:, :, None] > 0, t.astype(np.int64).astype(np.uint8), img[y0:y0 + ch, x0:x0 + cw])
    return out, t, A, raw


def eps_of(R, ch, cw):
    (_, wx), (_, wy) = inpaint.bicubic_weights(R, cw), inpaint.bicubic_weights(R, ch)
    return 255.0 * (wx.shape[1] + wy.shape[1] + 10) * 2.0 ** -24 * np.abs(wy).sum(1).max() * np.abs(wx).sum(1).max()


def byte_rule(got, img, mask, window, fake, feather):
    """Hold ``got`` uint8 [h, w, 3] to the rule above -> (share of window pixels left out of the equality, bytes that differ at all)."""
    y0, x0, ch, cw = window
    want, t, A, raw = paste_reference(img, mask, window, fake, feather, np.float64)
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8
    outside = np.ones(want.shape[:2], bool)
    outside[y0:y0 + ch, x0:x0 + cw] = False
    assert np.array_equal(got[outside], np.asarray(img)[outside]), 'a byte outside the window changed'
    g, w = got[y0:y0 + ch, x0:x0 + cw].astype(np.int64), want[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
    assert np.abs(g - w).max() <= 1, 'a byte is off by more than 1'
    assert np.array_equal(g[A == 0], w[A == 0]), 'a byte with A = 0 is not the original'
    eps = eps_of(np.asarray(fake).shape[-1], ch, cw) * max(1.0, float(np.abs(fake).max()))
    clamped = (raw <= -eps) | (raw >= 255.0 + eps)
    near = (np.abs(t - np.rint(t)) <= eps) & (A[:, :, None] > 0) & ~clamped
    assert np.array_equal(g[~near], w[~near]), f'{int((g != w)[~near].sum())} bytes differ farther than eps = {eps:.3e} from an integer'
    share = float(near.any(axis=2).sum()) / (ch * cw)
    assert share <= CAP, f'{share:.4%} of the window pixels lie within eps of an integer (cap {CAP:.0%})'
    return share, int((g != w).sum())


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------

def random_image(rng, h, w):
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def mask_with_holes(h, w, boxes):
    """uint8 [h, w] of ones with the (ya, yb, xa, xb) boxes zeroed."""
    m = np.ones((h, w), np.uint8)
    for ya, yb, xa, xb in boxes:
        m[ya:yb, xa:xb] = 0
    return m


# (h, w, hole boxes, window) at R = 16.  16 x 16 full window: the identity.  37 x 53, 9 x 70 (an axis below R: that axis is resampled
# down on the way back), 150 x 201 (a window several tiles wide and tall at the kernel's 16 x 128 tile, holes across the seams at row 16 /
# 32 and column 128 of the window).  Windows at (0, 0) and at the bottom-right corner; holes on the window's edges and corners; a one-pixel
# hole; odd sizes, so that image and mask offsets in a packed batch are no multiples of 4.
CASES = [
    (16, 16, [(5, 11, 4, 9)], (0, 0, 16, 16)),
    (37, 53, [(0, 6, 0, 9), (20, 21, 30, 31)], (0, 0, 37, 53)),
    (37, 53, [(30, 37, 45, 53)], (5, 13, 32, 40)),
    (37, 53, [(10, 18, 11, 29), (0, 2, 0, 3)], (3, 7, 29, 31)),                      # (a hole outside the window: left alone)
    (9, 70, [(2, 5, 30, 41)], (0, 17, 9, 40)),
    (9, 70, [(8, 9, 69, 70), (0, 1, 35, 36)], (0, 35, 9, 35)),
    (150, 201, [(10, 40, 120, 140), (14, 18, 0, 3), (31, 33, 60, 61), (100, 150, 190, 201)], (0, 0, 150, 201)),
    (150, 201, [(60, 90, 20, 170)], (17, 9, 120, 180)),
    (150, 201, [(149, 150, 200, 201)], (101, 151, 49, 50)),
    (150, 201, [(5, 140, 100, 104)], (3, 31, 147, 139)),
    (41, 23, [(0, 41, 0, 23)], (0, 0, 41, 23)),
    (33, 35, [(16, 17, 17, 18)], (7, 9, 19, 21)),
]


def make_case(idx, R=16, k=1):
    """-> (img, mask, window, fake float32 [k, 3, R, R] uniform in [-0.6, 0.6]) of CASES[idx], seeded."""
    h, w, boxes, window = CASES[idx]
    rng = np.random.RandomState(100 + idx)
    return random_image(rng, h, w), mask_with_holes(h, w, boxes), window, rng.uniform(-0.6, 0.6, (k, 3, R, R)).astype(np.float32)
