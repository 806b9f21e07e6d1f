"""CPU (no GPU): the float64 yardstick of the gradient-domain paste-back (tests/membrane_f64.py) against scipy and against closed forms,
``membrane_plan``'s integers, the new symbols, the float32 margin of the GPU suite's solver cases and ``Inpainter(blend=...)`` on the host."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import inpaint_f64 as ref
import membrane_f64 as mref
import test_inpaint_cpu as tic
from conftest import ROOT
from shgan_amd import _lib, inpaint

NEW = ('shg_inpaint_membrane_setup_f32', 'shg_membrane_solve_f32', 'shg_inpaint_membrane_paste_u8', 'shg_membrane_workspace_bytes',
       'shg_membrane_tile', 'shg_membrane_coarsest')
R = 16


# ------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ('blob', 'corridor', 'edge'))
def test_yardstick_equals_a_sparse_direct_solve(name):
    sp = pytest.importorskip('scipy.sparse')
    spl = pytest.importorskip('scipy.sparse.linalg')
    h, w = 23, 31
    om = mref.domain(name, h, w)
    field = mref.random_field(om, 3)[:, :, 0].astype(np.float64)
    idx = -np.ones((h, w), np.int64)
    idx[om] = np.arange(om.sum())
    rows, cols, vals, b = [], [], [], np.zeros(int(om.sum()))
    for y, x in zip(*np.nonzero(om)):
        rows.append(idx[y, x]), cols.append(idx[y, x]), vals.append(4.0)
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w:
                if om[yy, xx]:
                    rows.append(idx[y, x]), cols.append(idx[yy, xx]), vals.append(-1.0)
                else:
                    b[idx[y, x]] += field[yy, xx]
    want = spl.spsolve(sp.csr_matrix((vals, (rows, cols)), shape=(b.size, b.size)), b)
    got = mref.solve_reference(field, om)
    assert np.abs(got[om] - want).max() <= 1e-8 and np.array_equal(got[~om], field[~om])


def test_yardstick_analytic_cases():
    h, w = 19, 27
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    om = mref.domain('blob', h, w)                                              # does not touch the grid edge
    const = np.where(om, 0.0, 7.25)
    assert np.abs(mref.solve_reference(const, om) - 7.25).max() <= 1e-9        # d = delta -> c = delta
    plane = 0.75 * xx - 1.5 * yy + 3.0
    got = mref.solve_reference(np.where(om, 0.0, plane), om)
    assert np.abs(got - plane).max() <= 1e-9                                   # a plane is discrete-harmonic
    one = np.zeros((h, w), bool)
    one[5, 6] = True
    f = mref.random_field(one, 1)
    got = mref.solve_reference(f, one)
    want = (f[4, 6].astype(np.float64) + f[6, 6] + f[5, 5] + f[5, 7]) / 4
    assert np.abs(got[5, 6] - want).max() <= 1e-12
    # a pixel at the grid's corner: the two neighbours outside the grid count as 0
    corner = np.zeros((h, w), bool)
    corner[0, 0] = True
    f = mref.random_field(corner, 2)
    assert np.abs(mref.solve_reference(f, corner)[0, 0] - (f[1, 0].astype(np.float64) + f[0, 1]) / 4).max() <= 1e-12
    assert mref.residual_f64(got, one) <= 1e-12 and mref.residual_f64(f, corner) > 1e-3
    lo, hi = mref.byte_window(np.array([3.2, 3.9, 4.0]), 0.25)
    assert lo.tolist() == [2, 3, 3] and hi.tolist() == [3, 4, 4]


def test_the_solver_cases_leave_float32_a_margin_of_ten():
    """The GPU suite asserts residual_f64(device field) (n + 1)^2 / 8 <= tol.  That is reachable only if float32 can hold a field with so
    small a residual: the float64 solution rounded to float32 must meet it with a margin of at least 10 on every case."""
    worst = 0.0
    for name, h, w, seed in mref.solver_cases(inpaint.MEMBRANE_TILE, inpaint.MEMBRANE_COARSEST):
        om = mref.domain(name, h, w)
        f = mref.random_field(om, seed)
        c32 = mref.solve_reference(f, om).astype(np.float32)
        n = mref.omega_box_side(om)
        assert n <= 100
        bound = mref.residual_f64(c32, om) * (n + 1) ** 2 / 8
        worst = max(worst, bound)
        assert bound <= 0.25 / 10, (name, h, w, bound)
    print(f'largest certified error of a float32-rounded solution: {worst:.3e} grey levels')


# ------------------------------------------------------------------------------------------------
# the plan
# ------------------------------------------------------------------------------------------------

def test_membrane_plan_integers():
    shapes = np.array([[150, 201, 0], [37, 53, 150 * 201 * 3]])
    windows = np.array([[17, 9, 120, 180], [0, 0, 37, 53]])
    boxes = np.array([[60 + 17, 90 + 17, 20 + 9, 170 + 9], [30, 37, 45, 53]])   # image coordinates
    for feather, k in ((0, 1), (5, 3), (32, 2)):
        plan = inpaint.membrane_plan(shapes, windows, feather, k, boxes)
        assert plan.grids.dtype == np.int32 and plan.table.dtype == np.int32 and plan.table.shape == (2 * k, 4)
        for i, ((y0, x0, ch, cw), (ya, yb, xa, xb)) in enumerate(zip(windows, boxes)):
            oa, ob, pa, pb = max(ya - y0 - feather, 0), min(yb - y0 + feather, ch), max(xa - x0 - feather, 0), min(xb - x0 + feather, cw)
            gy0, gx0, gh, gw, foff, ooff = plan.grids[i]
            assert (gy0, gx0) == (max(oa - 1, 0), max(pa - 1, 0)) and (gy0 + gh, gx0 + gw) == (min(ob + 1, ch), min(pb + 1, cw))
            for j in range(k):
                assert tuple(plan.table[i * k + j]) == (gh, gw, foff + j * 3 * gh * gw, ooff)                # a shared Omega offset
                assert plan.n[i * k + j] == min(ob - oa, pb - pa)
            assert foff % 4 == 0 and foff + 3 * k * gh * gw <= plan.g_elems and ooff + gh * gw <= plan.omega_bytes
        g0, g1 = plan.grids
        assert g1[4] >= g0[4] + 3 * k * g0[2] * g0[3] and g1[5] >= g0[5] + g0[2] * g0[3]                    # disjoint
        assert (plan.max_h, plan.max_w) == (plan.grids[:, 2].max(), plan.grids[:, 3].max())
        assert plan.ws_bytes == inpaint.membrane_workspace_bytes(2 * k, plan.max_h, plan.max_w) > 12 * k * 2 * plan.max_h * plan.max_w
    whole = inpaint.membrane_plan(shapes, windows, 8, 1)                                                    # no boxes: the window
    assert [tuple(g[:4]) for g in whole.grids] == [(0, 0, 120, 180), (0, 0, 37, 53)] and whole.n.tolist() == [120, 37]
    with pytest.raises(ValueError):
        inpaint.membrane_plan(shapes, windows, 33, 1)
    with pytest.raises(ValueError):
        inpaint.membrane_plan(shapes, windows, 8, 1, np.array([[0, 5, 0, 5], [30, 37, 45, 53]]))            # a box that misses its window


# ------------------------------------------------------------------------------------------------
# the C-ABI
# ------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name)
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40
    assert lib.shg_membrane_tile() == inpaint.MEMBRANE_TILE and lib.shg_membrane_coarsest() == inpaint.MEMBRANE_COARSEST
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    p = ctypes.c_void_p(4096)

    def setup(src=p, mask=p, table=p, grids=p, fake=p, g=p, field=p, omega=p, g_elems=4096, om=4096, B=1, K=1, Rr=16, feather=8, chunks=1, bands=1,
              lds=1024):                                                                  # (every call fails a check: nothing is launched)
        return lib.shg_inpaint_membrane_setup_f32(src, 4096, mask, 4096, table, 4096, grids, fake, g, field, g_elems, omega, om, B, K, Rr, feather,
                                                  chunks, bands, lds, None)

    def paste(out=p, mask=p, table=p, grids=p, g=p, field=p, g_elems=4096, B=1, K=1, Rr=16, feather=8, chunks=1, bands=1, lds=1024):
        return lib.shg_inpaint_membrane_paste_u8(out, 4096, mask, 4096, table, 4096, grids, g, field, g_elems, None, B, K, Rr, feather, chunks, bands,
                                                 lds, None)

    def solve(field=p, omega=p, table=p, tol=p, ws=p, info=p, field_elems=4096, om=4096, P=1, cycles=4, mh=8, mw=8, ws_bytes=1 << 20):
        return lib.shg_membrane_solve_f32(field, field_elems, omega, om, table, P, tol, cycles, mh, mw, ws, ws_bytes, info, None)
    for kw in (dict(src=None), dict(mask=None), dict(table=None), dict(grids=None), dict(fake=None), dict(g=None), dict(field=None), dict(omega=None)):
        assert setup(**kw) == -1 and 'null' in err(), kw
    for kw in (dict(out=None), dict(mask=None), dict(table=None), dict(grids=None), dict(g=None), dict(field=None)):
        assert paste(**kw) == -1 and 'null' in err(), kw
    for kw in (dict(field=None), dict(omega=None), dict(table=None), dict(tol=None), dict(ws=None), dict(info=None)):
        assert solve(**kw) == -1 and 'null' in err(), kw
    for fn in (setup, paste):
        assert fn(Rr=0) == -1 and 'R must' in err()
        assert fn(K=0) == -1 and 'K must' in err()
        assert fn(B=0) == -1 and 'B must' in err()
        assert fn(B=300) == -1 and 'descriptors' in err()
        assert fn(lds=49153) == -1 and 'lds_bytes' in err()
        assert fn(g_elems=2) == -1 and 'g_elems' in err()
        for f in (-1, 33):
            assert fn(feather=f) == -1 and 'feather' in err()
    assert setup(om=0) == -1 and 'omega_bytes' in err()
    assert solve(P=0) == -1 and 'P must' in err()
    assert solve(cycles=-1) == -1 and solve(cycles=1025) == -1 and 'max_cycles' in err()
    assert solve(mh=0) == -1 and solve(mw=16385) == -1 and 'max_h' in err()
    assert solve(field_elems=2) == -1 and 'field_elems' in err()
    need = lib.shg_membrane_workspace_bytes(3, 100, 70)
    assert need > 3 * 12 * 100 * 70 and need % 16 == 0
    assert solve(P=3, mh=100, mw=70, ws_bytes=need - 1) == -1 and 'workspace' in err()
    assert solve(field=ctypes.c_void_p(4100)) == -1 and 'aligned' in err()
    assert lib.shg_membrane_workspace_bytes(0, 8, 8) == 0 and lib.shg_membrane_workspace_bytes(1, 0, 8) == 0
    # the workspace grows with either side (a slice sized for the largest grid holds every smaller one)
    sizes = [lib.shg_membrane_workspace_bytes(1, h, 50) for h in range(1, 140)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


# ------------------------------------------------------------------------------------------------
# Inpainter on the host
# ------------------------------------------------------------------------------------------------

def _paste_membrane_ref(packed, packed_mask, shapes, windows, fake, k=1, feather=8):
    pk, pm, fake = packed.numpy(), packed_mask.numpy(), fake.numpy()
    out = np.stack([pk] * k)
    for n, ((h, w, off, moff), window) in enumerate(zip(shapes, windows)):
        for j in range(k):
            res = mref.paste_reference(pk[off:off + 3 * h * w].reshape(h, w, 3), pm[moff:moff + h * w].reshape(h, w), tuple(int(v) for v in window),
                                       fake[n * k + j], feather)[0]
            out[j, off:off + 3 * h * w] = res.reshape(-1)
    return torch.from_numpy(out)


def test_inpainter_blend_on_the_host():
    rng = np.random.RandomState(4)
    sizes = [(37, 53), (20, 20), (33, 35)]
    images = [ref.random_image(rng, h, w) for h, w in sizes]
    masks = [ref.mask_with_holes(37, 53, [(10, 18, 11, 29)]), np.ones((20, 20), np.uint8), ref.mask_with_holes(33, 35, [(16, 17, 17, 18)])]
    z = torch.from_numpy(rng.standard_normal((3, 2, 4)).astype(np.float32))
    kw = dict(feather=2, batch=2, gather_fn=tic._gather_ref)
    today = inpaint.Inpainter(tic.StandInG(), R, 'cpu', paste_fn=tic._paste_ref, **kw)(images, masks, z=z[:, 0])
    feather = inpaint.Inpainter(tic.StandInG(), R, 'cpu', paste_fn=tic._paste_ref, blend='feather', **kw)
    assert feather.blend == 'feather' and feather.paste_fn is tic._paste_ref
    assert all(np.array_equal(a, b) for a, b in zip(today, feather(images, masks, z=z[:, 0])))
    assert inpaint.Inpainter(tic.StandInG(), R, 'cpu').paste_fn is inpaint.paste_back
    assert inpaint.Inpainter(tic.StandInG(), R, 'cpu', blend='membrane').paste_fn is inpaint.paste_back_membrane
    mem = inpaint.Inpainter(tic.StandInG(), R, 'cpu', paste_fn=_paste_membrane_ref, blend='membrane', **kw)
    res = mem(images, masks, z=z[:, 0])
    assert np.array_equal(res[1], images[1])
    for i in (0, 2):
        window = inpaint.plan_window(masks[i], R, 0.5, 2)
        A = ref.feather_reference(masks[i][window[0]:window[0] + window[2], window[1]:window[1] + window[3]], 2)
        keep = np.ones(sizes[i], bool)
        keep[window[0]:window[0] + window[2], window[1]:window[1] + window[3]] = A == 0
        assert res[i].shape == images[i].shape and np.array_equal(res[i][keep], images[i][keep])
        assert not np.array_equal(res[i], images[i]) and not np.array_equal(res[i], today[i])
    res2 = mem(images, masks, z=z, samples=2)
    assert [r.shape for r in res2] == [(2,) + im.shape for im in images] and np.array_equal(res2[0][0], res[0])
    for bad in ('poisson', None, ''):
        with pytest.raises(ValueError, match='blend'):
            inpaint.Inpainter(tic.StandInG(), R, 'cpu', blend=bad)
