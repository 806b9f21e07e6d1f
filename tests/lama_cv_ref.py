"""Yardstick of the LaMa-mask tests: OpenCV 4.x ``cv2.line(img, p0, p1, 1, thickness)`` for thickness > 1 (``ThickLine`` ->
``FillConvexPoly`` + ``Line2`` + ``clipLine`` + filled ``Circle``, 16.16 fixed point), restated in plain Python integers from the
algorithm, row by row and pixel by pixel as the library walks them.  Its agreement with an actual ``cv2`` is checked only where
``cv2`` imports (tests/test_lama_cpu.py); the device kernel (csrc/mask_lama.hip) and the host path (masks.lama_draw_host) must equal
THIS file bit for bit.  Python ints are unbounded (the specification's 64-bit integers never overflow here), ``>>`` on them is
arithmetic, floats are IEEE doubles and ``round`` rounds half to even (``cvRound``)."""
import math
import sys

import numpy as np

XS = 16
ONE = 1 << XS
HALF = ONE >> 1
TRACE = None        # a set: clip_line adds the label of every branch it takes (tests that must reach every branch read it)


def _trace(label):
    if TRACE is not None:
        TRACE.add(label)


def tdiv(a, b):
    """C integer division: truncates toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def clip_line(w, h, x1, y1, x2, y2):
    """``clipLine((w, h), p1, p2)`` -> (accepted, x1, y1, x2, y2)."""
    right, bottom = w - 1, h - 1

    def code(x, y):
        return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8

    c1, c2 = code(x1, y1), code(x2, y2)
    _trace('inside' if (c1 | c2) == 0 else 'same side' if (c1 & c2) else 'clipped')
    went_in = (c1 & c2) == 0 and (c1 | c2) != 0
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            _trace('p1 top' if c1 < 8 else 'p1 bottom')
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            _trace('p2 top' if c2 < 8 else 'p2 bottom')
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                _trace('p1 left' if c1 == 1 else 'p1 right')
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                _trace('p2 left' if c2 == 1 else 'p2 right')
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    if went_in and (c1 | c2) != 0:
        _trace('rejected after clipping')
    return (c1 | c2) == 0, x1, y1, x2, y2


def _put(img, x, y):
    if 0 <= x < img.shape[1] and 0 <= y < img.shape[0]:
        img[y, x] = 1


def line2(img, a, b):
    """``Line2``: the outline walk between two 16.16 points."""
    h, w = img.shape
    ok, x1, y1, x2, y2 = clip_line(w << XS, h << XS, a[0], a[1], b[0], b[1])
    if not ok:
        return
    dx, dy = x2 - x1, y2 - y1
    ax, ay = abs(dx), abs(dy)
    if ax > ay:
        if dx < 0:
            x1, y1, x2, y2, dy = x2, y2, x1, y1, -dy
        step = tdiv(dy << XS, ax | 1)
        n = (x2 - x1) >> XS
    else:
        if dy < 0:
            x1, y1, x2, y2, dx = x2, y2, x1, y1, -dx
        step = tdiv(dx << XS, ay | 1)
        n = (y2 - y1) >> XS
    x1 += HALF
    y1 += HALF
    _put(img, (x2 + HALF) >> XS, (y2 + HALF) >> XS)
    if ax > ay:
        px = x1 >> XS
        for _ in range(n + 1):
            _put(img, px, y1 >> XS)
            px += 1
            y1 += step
    else:
        py = y1 >> XS
        for _ in range(n + 1):
            _put(img, x1 >> XS, py)
            py += 1
            x1 += step


def fill_convex(img, v):
    """``FillConvexPoly`` of the four 16.16 vertices ``v``."""
    h, w = img.shape
    for i, j in ((3, 0), (0, 1), (1, 2), (2, 3)):
        line2(img, v[i], v[j])
    xs_, ys_ = [p[0] for p in v], [p[1] for p in v]
    imin = ys_.index(min(ys_))
    xmin, xmax = (min(xs_) + HALF) >> XS, (max(xs_) + HALF) >> XS
    ymin, ymax = (min(ys_) + HALF) >> XS, (max(ys_) + HALF) >> XS
    if xmax < 0 or ymax < 0 or xmin >= w or ymin >= h:
        return
    ymax = min(ymax, h - 1)
    idx, di = [imin, imin], [1, 3]
    x, dx, ye = [-ONE, -ONE], [0, 0], [ymin, ymin]
    edges = 4
    for y in range(ymin, ymax + 1):
        for i in range(2):
            if y >= ye[i]:
                idx0 = idx[i]
                k = (idx0 + di[i]) % 4
                while True:
                    go = edges > 0
                    edges -= 1
                    if not go:
                        break
                    ty = (v[k][1] + HALF) >> XS
                    if ty > y:
                        xs, xe = v[idx0][0], v[k][0]
                        ye[i] = ty
                        dx[i] = tdiv((xe - xs) * 2 + (ty - y), 2 * (ty - y))
                        x[i] = xs
                        idx[i] = k
                        break
                    idx0 = k
                    k = (k + di[i]) % 4
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if x[0] > x[1] else (0, 1)
            xx1, xx2 = (x[left] + HALF) >> XS, (x[right] + HALF) >> XS
            if xx2 >= 0 and xx1 < w:
                xx1, xx2 = max(xx1, 0), min(xx2, w - 1)
                if xx1 <= xx2:
                    img[y, xx1:xx2 + 1] = 1
        x[0] += dx[0]
        x[1] += dx[1]


def _hline(img, y, xa, xb):
    h, w = img.shape
    if 0 <= y < h:
        xa, xb = max(xa, 0), min(xb, w - 1)
        if xa <= xb:
            img[y, xa:xb + 1] = 1


def circle(img, cx, cy, r):
    """Filled ``Circle``: the midpoint walk, four spans per step, each clipped to the canvas."""
    err, dx, dy, plus, minus = 0, r, 0, 1, (r << 1) - 1
    while dx >= dy:
        _hline(img, cy - dy, cx - dx, cx + dx)
        _hline(img, cy + dy, cx - dx, cx + dx)
        _hline(img, cy - dx, cx - dy, cx + dy)
        _hline(img, cy + dx, cx - dy, cx + dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2


def line(img, p0, p1, t):
    """``cv2.line(img, p0, p1, 1, t)`` for t > 1 on a 2-D uint8 array, in place."""
    if t <= 1:
        raise ValueError('lama_cv_ref.line: thickness must be > 1')
    a = (int(p0[0]) << XS, int(p0[1]) << XS)
    b = (int(p1[0]) << XS, int(p1[1]) << XS)
    dx, dy = (a[0] - b[0]) / 65536.0, (b[1] - a[1]) / 65536.0
    r = dx * dx + dy * dy
    odd, T = t & 1, t << (XS - 1)
    if abs(r) > sys.float_info.epsilon:
        r = (T + odd * ONE * 0.5) / math.sqrt(r)
        dpx, dpy = round(dy * r), round(dx * r)
        fill_convex(img, [(a[0] + dpx, a[1] + dpy), (a[0] - dpx, a[1] - dpy), (b[0] - dpx, b[1] - dpy), (b[0] + dpx, b[1] + dpy)])
    for p in (a, b):
        circle(img, (p[0] + HALF) >> XS, (p[1] + HALF) >> XS, (T + HALF) >> XS)


def draw(calls, s):
    """Painted pixels (uint8 [s,s], 1 = painted) of a list of ``(x0, y0, x1, y1, t)`` calls."""
    img = np.zeros((s, s), np.uint8)
    for x0, y0, x1, y1, t in calls:
        line(img, (int(x0), int(y0)), (int(x1), int(y1)), int(t))
    return img


def capsule_distance(s, p0, p1):
    """float64 [s,s]: distance of every pixel centre (x, y) to the segment p0-p1."""
    yy, xx = np.mgrid[0:s, 0:s].astype(np.float64)
    ax, ay, bx, by = float(p0[0]), float(p0[1]), float(p1[0]), float(p1[1])
    vx, vy = bx - ax, by - ay
    l2 = vx * vx + vy * vy
    u = np.zeros_like(xx) if l2 == 0 else np.clip(((xx - ax) * vx + (yy - ay) * vy) / l2, 0.0, 1.0)
    return np.hypot(xx - (ax + u * vx), yy - (ay + u * vy))


def random_segments(seed=11):
    """The 800 segments of the capsule / cv2 tests: 400 at s = 64 and 400 at s = 256, thickness 5 .. 104, end points in [0, s] inclusive
    (one past the canvas, as the reference's clip allows), one in five of near-zero length (each coordinate moves by -1, 0 or 1)
    -> list of (s, x0, y0, x1, y1, t)."""
    rs = np.random.RandomState(seed)
    out = []
    for s in (64, 256):
        for i in range(400):
            t = int(rs.randint(5, 105))
            x0, y0 = (int(v) for v in rs.randint(0, s + 1, size=2))
            if i % 5 == 0:
                x1, y1 = (int(np.clip(c + rs.randint(-1, 2), 0, s)) for c in (x0, y0))
            else:
                x1, y1 = (int(v) for v in rs.randint(0, s + 1, size=2))
            out.append((s, x0, y0, x1, y1, t))
    return out
