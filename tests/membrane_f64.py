"""Yardstick of the gradient-domain paste-back (sh-gan_amd/inpaint.py ``paste_back_membrane``, csrc/membrane.hip): the membrane in float64
by conjugate gradients, an independent residual, the float64 restatement of the whole chain and the byte window a device result is held
to.  Numpy only; nothing here is shipped.

THE DISCRETE PROBLEM.  ``field`` [h, w] or [h, w, C], ``omega`` [h, w] (non-zero = unknown).  Find c with c = field outside Omega and
4 c(p) - sum_{q in N4(p)} c(q) = 0 for p in Omega, neighbours outside the h x w grid counting as 0.  The matrix (the 5-point Laplacian
restricted to Omega) is symmetric positive definite whatever Omega is: every component is anchored by the Dirichlet data around it.

THE BOUND.  With r the residual of an approximation c~ and n the shorter side of Omega's bounding box, |c~ - c| <= max|r| (n + 1)^2 / 8:
the comparison function (x - a + 1)(b + 1 - x) / 2 along that side (a..b the box) has discrete Laplacian -1... i.e. 4 w - sum = 1 in
Omega, is >= 0 outside, and peaks at (n + 1)^2 / 8; the discrete maximum principle does the rest.

THE BYTE WINDOW of the whole chain.  v64 is the float64 pre-truncation value of the restated chain.  A device result carries the float32
error of the resample chain and the blend (``inpaint_f64.eps_of`` bounds it by eps, with the slack derived there: the chain's own
error is about a third of eps, which leaves room for the same error entering once more through d = orig - g and the membrane, a convex
combination of its Dirichlet values) and at most tol in c; clamp and the convex blend do not amplify: the device's pre-truncation value
lies within eps + tol of v64, and its byte in ``byte_window(v64, eps + tol)``."""
import numpy as np

import inpaint_f64 as ref


def _nbsum(u):
    p = np.pad(u, ((1, 1), (1, 1)) + ((0, 0),) * (u.ndim - 2))
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]


def residual_f64(field, omega):
    """max over Omega (and channels) of |4 c - sum of the four neighbours| in float64, by explicit loops over the neighbours' shifts --
    written apart from ``solve_reference``'s operator."""
    c = np.asarray(field, np.float64)
    om = np.asarray(omega) != 0
    h, w = om.shape
    worst = 0.0
    ys, xs = np.nonzero(om)
    acc = 4.0 * c[ys, xs]
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        y, x = ys + dy, xs + dx
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        nb = np.zeros_like(acc)
        nb[ok] = c[y[ok], x[ok]]
        acc = acc - nb
    if acc.size:
        worst = float(np.abs(acc).max())
    return worst


def solve_reference(field, omega, rtol=1e-10, max_iter=100000):
    """-> float64 array of field's shape: c in Omega, field elsewhere.  Conjugate gradients on the unknowns of Omega until the residual's
    max norm is <= rtol."""
    f = np.asarray(field, np.float64)
    squeeze = f.ndim == 2
    if squeeze:
        f = f[:, :, None]
    om = np.asarray(omega) != 0
    m3 = om[:, :, None]
    bdry = np.where(m3, 0.0, f)
    b = np.where(m3, _nbsum(bdry), 0.0)                       # 4 c - sum over unknown neighbours = sum over known neighbours

    def A(x):
        return np.where(m3, 4.0 * x - _nbsum(x), 0.0)
    x = np.zeros_like(f)
    r = b - A(x)
    p = r.copy()
    rs = (r * r).sum(axis=(0, 1))
    for _ in range(max_iter):
        if np.abs(r).max() <= rtol:
            break
        Ap = A(p)
        den = (p * Ap).sum(axis=(0, 1))
        alpha = np.where(den > 0, rs / np.where(den > 0, den, 1.0), 0.0)
        x = x + alpha * p
        r = r - alpha * Ap
        rs_new = (r * r).sum(axis=(0, 1))
        beta = np.where(rs > 0, rs_new / np.where(rs > 0, rs, 1.0), 0.0)
        p = r + beta * p
        rs = rs_new
    out = np.where(m3, x, f)
    assert residual_f64(out, om) <= 10 * rtol, 'the yardstick did not converge'
    return out[:, :, 0] if squeeze else out


def omega_box_side(omega):
    """The shorter side of Omega's bounding box (the n of the bound), 0 for an empty Omega."""
    om = np.asarray(omega) != 0
    rows, cols = np.flatnonzero(om.any(axis=1)), np.flatnonzero(om.any(axis=0))
    return 0 if rows.size == 0 else int(min(rows[-1] - rows[0] + 1, cols[-1] - cols[0] + 1))


def setup_reference(img, mask, window, fake, feather, dtype=np.float64):
    """One image, one sample -> (g [ch, cw, 3] = clamp(v 127.5 + 127.5) in ``dtype``, field [ch, cw, 3] = orig - g where A = 0 and 0 in
    Omega, omega bool [ch, cw] = A > 0, A uint8 [ch, cw]) over the whole window."""
    y0, x0, ch, cw = window
    A = ref.feather_reference(np.asarray(mask)[y0:y0 + ch, x0:x0 + cw], feather)
    v = ref.resample_reference(fake, ch, cw, dtype).transpose(1, 2, 0)
    c = dtype(127.5)
    g = np.clip(v * c + c, dtype(0), dtype(255))
    orig = np.asarray(img, np.uint8)[y0:y0 + ch, x0:x0 + cw].astype(dtype)
    omega = A > 0
    field = np.where(omega[:, :, None], dtype(0), orig - g).astype(dtype)
    return g, field, omega, A


def paste_reference(img, mask, window, fake, feather, c=None):
    """The whole chain in float64 -> (result uint8 [h, w, 3], t [ch, cw, 3] the pre-truncation values, A, c64 [ch, cw, 3] the membrane on
    the window).  ``c``: a membrane to use in place of the yardstick's (the paste step alone)."""
    y0, x0, ch, cw = window
    img = np.asarray(img, np.uint8)
    F = float(feather + 1)
    g, field, omega, A = setup_reference(img, mask, window, fake, feather, np.float64)
    if c is None:
        c = solve_reference(field, omega)
    u = np.clip(g + np.asarray(c, np.float64), 0.0, 255.0)
    a = A[:, :, None].astype(np.float64)
    orig = img[y0:y0 + ch, x0:x0 + cw].astype(np.float64)
    t = (a * u + (F - a) * orig) / F
    out = img.copy()
    out[y0:y0 + ch, x0:x0 + cw] = np.where(A[:, :, None] > 0, t.astype(np.int64).astype(np.uint8), img[y0:y0 + ch, x0:x0 + cw])
    return out, t, A, c


def byte_window(v64, tau):
    """-> (lo, hi) int64: the bytes a value within tau of v64 can truncate to."""
    v = np.asarray(v64, np.float64)
    return np.floor(v - tau).astype(np.int64), np.floor(v + tau).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# domains of the solver's tests: (h, w) -> bool [h, w]
# ------------------------------------------------------------------------------------------------

def domain(name, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    m = min(h, w)
    if name == 'blob':                               # an ellipse with two discs carved out; does not touch the grid edge
        om = ((yy - h / 2) ** 2 / (h * 0.42) ** 2 + (xx - w / 2) ** 2 / (w * 0.42) ** 2) < 1
        om &= ((yy - h * 0.4) ** 2 + (xx - w * 0.35) ** 2) > (m * 0.12) ** 2
        om &= ((yy - h * 0.7) ** 2 + (xx - w * 0.65) ** 2) > (m * 0.08) ** 2
        om[0] = om[-1] = False
        om[:, 0] = om[:, -1] = False
    elif name == 'two':                              # two disjoint components
        om = np.zeros((h, w), bool)
        om[2:h // 2 - 1, 2:w // 2 - 2] = True
        om[h // 2 + 2:h - 2, w // 2 + 1:w - 3] = True
    elif name == 'edge':                             # touches the grid's edges and two corners
        om = np.zeros((h, w), bool)
        om[0:h // 2, 0:w // 3] = True
        om[h // 3:, w // 2:] = True
        om[h - 3:, :] = True
    elif name == 'corridor':                         # two blobs joined by a corridor one pixel wide
        om = np.zeros((h, w), bool)
        om[3:h // 3, 3:w // 3] = True
        om[2 * h // 3:h - 3, 2 * w // 3:w - 3] = True
        om[h // 4, w // 3:5 * w // 6] = True
        om[h // 4:2 * h // 3, 5 * w // 6] = True
    elif name == 'full':                             # the whole rectangle
        om = np.ones((h, w), bool)
    elif name == 'inner':                            # a full rectangle inside a ring of data
        om = np.zeros((h, w), bool)
        om[1:h - 1, 1:w - 1] = True
    else:
        raise KeyError(name)
    return om


def solver_cases(T, C):
    """(domain, h, w, seed) of the solver's tests, T the smoother's tile side and C the coarsest level's largest side: grid sides T - 1, T,
    T + 1 (one tile, one tile exactly, a second tile of one cell), 2 T + 3 (three tiles) and 97 (>= three levels), every domain at
    every size; and grids smaller than C, which the one-workgroup kernel solves alone.  Omega's bounding box stays <= 100."""
    sizes = [(T - 1, T + 1), (T, T), (T + 1, T - 1), (2 * T + 3, T), (97, 2 * T + 3)]
    cases = [(name, h, w, 10 * i + j) for i, (h, w) in enumerate(sizes) for j, name in enumerate(('blob', 'two', 'edge', 'corridor', 'full', 'inner'))]
    cases += [('inner', C - 5, C - 3, 90), ('edge', C - 2, C, 91), ('blob', C, C - 1, 92)]
    return cases


def random_field(omega, seed, amp=32.0):
    """float32 [h, w, 3]: uniform in [-amp, amp] outside Omega, 0 inside."""
    rng = np.random.RandomState(seed)
    f = rng.uniform(-amp, amp, omega.shape + (3,)).astype(np.float32)
    f[omega] = 0.0
    return f
