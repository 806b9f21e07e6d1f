"""No GPU: the hole groups of sh-gan_amd/inpaint.py on the host -- the numpy yardstick tests/hole_groups_ref.py
against scipy, the three invariants that r = feather + 1 buys (checked before anything is built on them), ``plan_windows``' integers and
its fallback, the new symbols, and ``Inpainter(windows='per_hole')`` with injected reference functions and a stand-in G."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hole_groups_ref as hg
import inpaint_f64 as ref
from shgan_amd import _lib, eval_harness, inpaint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('shg_hole_label_tile', 'shg_hole_label_i32', 'shg_hole_owner_u8', 'shg_inpaint_paste_keyed_u8', 'shg_inpaint_membrane_setup_keyed_f32',
       'shg_inpaint_membrane_paste_keyed_u8')
R = 16


def test_reference_equals_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    T = 16
    masks = hg.random_masks(40, 11) + [m for r in (1, 4) for _, m in hg.single_cases(T, r)]
    for feather in (0, 3):
        r = feather + 1
        for m in masks:
            labels, comps = hg.groups_reference(m, feather)
            D = ndi.maximum_filter((m == 0).astype(np.uint8), size=2 * r + 1, mode='constant', cval=0) > 0
            assert np.array_equal(D, hg.dilate(m == 0, r))
            lab, n = ndi.label(D, structure=np.ones((3, 3)))
            assert n == comps.shape[0]
            flat = lab.reshape(-1)
            roots = np.full(n + 1, -1, np.int64)
            for i in np.flatnonzero(flat)[::-1]:                     # the smallest index of a label is written last
                roots[flat[i]] = i
            assert np.array_equal(roots[lab], labels)
            for c in comps:
                holes = (labels == c[1]) & (m == 0)
                assert ref.hole_box(np.where(holes, 0, 1)) == tuple(c[2:6]) and holes.sum() == c[6]


def _grow4(b):
    out = b.copy()
    out[1:] |= b[:-1]
    out[:-1] |= b[1:]
    out[:, 1:] |= b[:, :-1]
    out[:, :-1] |= b[:, 1:]
    return out


@pytest.mark.parametrize('feather', (0, 1, 5))
def test_what_r_equals_feather_plus_one_buys(feather):
    """On 200 seeded random masks: (1) the feather ring {A_j > 0} of a group and the ring's 4-neighbours (the membrane's Dirichlet rim) lie
    in the group's component of D; (2) on any row at least three pixels separate the rings of two groups; (3) the groups' weights sum to
    the weight of the whole mask over the whole image."""
    several = 0
    for m in hg.random_masks(200, 5):
        labels, comps = hg.groups_reference(m, feather)
        groups = hg.group_masks(m, feather)
        assert [g[0] for g in groups] == comps[:, 1].tolist()
        several += len(groups) > 1
        total = np.zeros(m.shape, np.int64)
        ring_of = np.zeros(m.shape, np.int64)
        for j, (root, gm) in enumerate(groups):
            A = ref.feather_reference(gm, feather)
            assert np.all(labels[_grow4(A > 0)] == root)                                   # (1)
            assert not np.any(ring_of[A > 0])
            ring_of[A > 0] = j + 1
            total += A
        assert np.array_equal(total, ref.feather_reference(m, feather))                    # (3)
        for row in ring_of:                                                                 # (2)
            xs = np.flatnonzero(row)
            other = row[xs[1:]] != row[xs[:-1]]
            assert np.all((xs[1:] - xs[:-1])[other] >= 4)
    assert several >= 20                                                                    # (the sweep does see images with several groups)


def test_plan_windows_integers_and_fallback():
    shapes = np.array([[300, 400, 0, 0], [50, 60, 360000, 120000], [90, 90, 369000, 123000]])
    comps = np.array([[2, 700, 10, 12, 70, 75, 9], [0, 5000, 10, 30, 200, 260, 900], [0, 90000, 250, 300, 0, 20, 800], [2, 100, 1, 2, 10, 11, 1],
                      [0, 40, 0, 1, 40, 41, 1]])
    plan = inpaint.plan_windows(comps, shapes, 64, 0.5, 8, max_windows=3)
    assert plan.image.tolist() == [0, 0, 0, 2, 2] and plan.key.tolist() == [1, 2, 3, 1, 2]
    assert plan.table.tolist() == [[0, 40, 1], [0, 5000, 2], [0, 90000, 3], [2, 100, 1], [2, 700, 2]]
    assert plan.boxes.tolist() == [[0, 1, 40, 41], [10, 30, 200, 260], [250, 300, 0, 20], [1, 2, 10, 11], [10, 12, 70, 75]]
    for i, box, window in zip(plan.image, plan.boxes, plan.windows):
        h, w = shapes[i, :2]
        m = ref.mask_with_holes(h, w, [tuple(box)])
        assert tuple(window) == inpaint.plan_window(m, 64, 0.5, 8) == inpaint.window_of_box(box, h, w, 64, 0.5, 8)
        ref.check_window(m, tuple(int(v) for v in window), 64, 0.5, 8)
    assert plan.windows.dtype == np.int64 and plan.windows[0].tolist() == [0, 8, 64, 64]
    # more groups than max_windows: the image is served by one window over all its holes, every group key 1
    plan = inpaint.plan_windows(comps, shapes, 64, 0.5, 8, max_windows=2)
    assert plan.image.tolist() == [0, 2, 2] and plan.key.tolist() == [1, 1, 2]
    assert plan.table.tolist() == [[0, 40, 1], [0, 5000, 1], [0, 90000, 1], [2, 100, 1], [2, 700, 2]]
    m = ref.mask_with_holes(300, 400, [(0, 1, 40, 41), (10, 30, 200, 260), (250, 300, 0, 20)])
    assert plan.boxes[0].tolist() == [0, 300, 0, 260] and tuple(plan.windows[0]) == inpaint.plan_window(m, 64, 0.5, 8)
    empty = inpaint.plan_windows(np.zeros((0, 7)), shapes, 64)
    assert empty.image.shape == (0,) and empty.windows.shape == (0, 4) and empty.table.shape == (0, 3)
    for bad in (0, 256):
        with pytest.raises(ValueError):
            inpaint.plan_windows(comps, shapes, 64, max_windows=bad)
    with pytest.raises(ValueError):
        inpaint.plan_windows(np.array([[3, 0, 0, 1, 0, 1, 1]]), shapes, 64)


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(raw, name)
    lib = _lib.get_lib()
    assert _lib.ABI_VERSION == 40 and lib.shg_abi_version() == 40
    assert inpaint.hole_label_tile() == lib.shg_hole_label_tile() and inpaint.hole_label_tile() >= 8
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    p = ctypes.c_void_p(4096)

    def label(mask=p, shapes=p, labels=p, scratch=p, comps=p, counter=p, B=1, mh=8, mw=8, r=1, cap=4):    # (every call fails a check: nothing is launched)
        return lib.shg_hole_label_i32(mask, 4096, shapes, B, mh, mw, r, cap, labels, scratch, comps, counter, None)

    def owner(mask=p, shapes=p, labels=p, table=p, scratch=p, own=p, B=1, n=1):
        return lib.shg_hole_owner_u8(mask, 4096, shapes, B, 8, 8, labels, table, n, scratch, own, None)
    for kw in (dict(mask=None), dict(shapes=None), dict(labels=None), dict(scratch=None), dict(comps=None), dict(counter=None)):
        assert label(**kw) == -1 and 'null' in err(), kw
    for kw in (dict(mask=None), dict(shapes=None), dict(labels=None), dict(table=None), dict(scratch=None), dict(own=None)):
        assert owner(**kw) == -1 and 'null' in err(), kw
    for r in (0, 34):
        assert label(r=r) == -1 and 'r must' in err()
    assert label(B=0) == -1 and 'B must' in err() and owner(B=0) == -1 and 'B must' in err()
    assert label(cap=0) == -1 and 'max_components' in err() and label(mh=0) == -1 and 'max_h' in err() and owner(n=-1) == -1 and 'n_table' in err()
    assert lib.shg_inpaint_paste_keyed_u8(p, 4096, p, 4096, None, p, 4096, p, None, 1, 1, 16, 8, 1, 1, 1024, None) == -1 and 'null' in err()
    assert lib.shg_inpaint_paste_keyed_u8(p, 4096, p, 4096, p, p, 4096, p, None, 1, 1, 16, 33, 1, 1, 1024, None) == -1 and 'feather' in err()
    assert lib.shg_inpaint_membrane_setup_keyed_f32(p, 4096, p, 4096, None, p, 4096, p, p, p, p, 4096, p, 4096, 1, 1, 16, 8, 1, 1, 1024, None) == -1
    assert 'null' in err()
    assert lib.shg_inpaint_membrane_paste_keyed_u8(p, 4096, p, 4096, None, p, 4096, p, p, p, 4096, None, 1, 1, 16, 8, 1, 1, 1024, None) == -1
    assert 'null' in err()


# ------------------------------------------------------------------------------------------------
# Inpainter(windows='per_hole') on the host
# ------------------------------------------------------------------------------------------------

class StandInG:
    """The image channels of x scaled, plus a z-dependent offset: enough to tell images, windows and samples apart."""
    z_dim, c_dim = 4, 0

    def __init__(self):
        self.calls = []

    def __call__(self, x, z, c, noise_mode='const'):
        self.calls.append(x.shape[0])
        return x[:, 1:] * 0.5 + z[:, :1, None, None] * 0.2

    def sample_many(self, x, z, c=None, noise_mode='random'):
        self.calls.append(x.shape[0])
        return x[:, None, 1:] * 0.5 + z[:, :, :1, None, None] * 0.2


def _gather_ref(packed, packed_mask, shapes, windows, Rr):
    pk, pm = packed.numpy(), packed_mask.numpy()
    real, mask = [], []
    for (h, w, off, moff), window in zip(shapes, windows):
        r, m = ref.gather_reference(pk[off:off + 3 * h * w].reshape(h, w, 3), pm[moff:moff + h * w].reshape(h, w), tuple(window), Rr)
        real.append(r)
        mask.append(m[None])
    return torch.from_numpy(np.stack(real)), torch.from_numpy(np.stack(mask))


def _paste_keyed_ref(packed, packed_mask, shapes, windows, fake, k=1, feather=8, owner=None, keys=None):
    """``paste_back``'s keyed form on the host: window n blends the holes whose owner byte is keys[n], into the running result."""
    assert owner is not None and len(keys) == len(windows)
    out, ow, fake = np.stack([packed.numpy()] * k), owner.numpy(), fake.numpy()
    for n, ((h, w, off, moff), window) in enumerate(zip(shapes, windows)):
        gm = np.where(ow[moff:moff + h * w].reshape(h, w) == keys[n], 0, 1)
        for j in range(k):
            cur = out[j, off:off + 3 * h * w].reshape(h, w, 3)
            out[j, off:off + 3 * h * w] = ref.paste_reference(cur, gm, tuple(int(v) for v in window), fake[n * k + j], feather, np.float32)[0].reshape(-1)
    return torch.from_numpy(out)


def _one_after_another(img, mask, z_row, feather, samples=None):
    """The expected result, written out: per group (in root order) ``plan_window`` of the group's own mask, the gather of the NATIVE
    mask, the stand-in G, the paste of the group's mask into the running image."""
    G, out = StandInG(), img.copy()
    for root, gm in hg.group_masks(mask, feather):
        window = inpaint.plan_window(gm, R, 0.5, feather)
        real, m = ref.gather_reference(img, mask, window, R)
        x = eval_harness.assemble_input(torch.from_numpy(real[None]), torch.from_numpy(m[None, None]))
        fake = G(x=x, z=z_row[None], c=z_row[None, :0]).float().numpy()[0]
        out = ref.paste_reference(out, gm, window, fake, feather, np.float32)[0]
    return out


def test_inpainter_per_hole_on_the_host():
    rng = np.random.RandomState(9)
    feather = 2
    sizes = [(70, 90), (20, 20), (40, 100), (33, 35)]
    images = [ref.random_image(rng, h, w) for h, w in sizes]
    masks = [ref.mask_with_holes(70, 90, [(5, 12, 6, 14), (50, 60, 70, 85), (52, 55, 60, 66), (30, 31, 40, 41)]), np.ones((20, 20), np.uint8),
             ref.mask_with_holes(40, 100, [(10, 20, 5, 15), (12, 18, 80, 95)]), ref.mask_with_holes(33, 35, [(16, 17, 17, 18)])]
    z = torch.from_numpy(rng.standard_normal((4, 4)).astype(np.float32))
    kw = dict(feather=feather, gather_fn=_gather_ref, paste_fn=_paste_keyed_ref, windows='per_hole', label_fn=hg.label_fn, owner_fn=hg.owner_fn)
    results = {}
    for batch in (1, 3):
        G = StandInG()
        inp = inpaint.Inpainter(G, R, 'cpu', batch=batch, **kw)
        results[batch] = inp(images, masks, z=z)
        # image 0: the holes at columns 60..65 and 70..84 are 4 < 2 r = 6 apart and share a group: three groups; image 2: two; image 3: one
        assert [(i, k) for i, k, _, _ in inp.windows_] == [(0, 1), (0, 2), (0, 3), (2, 1), (2, 2), (3, 1)]
        assert inp.windows_[2][3] == (50, 60, 60, 85)
        assert sum(G.calls) == 6 and max(G.calls) <= batch
    assert all(np.array_equal(a, b) for a, b in zip(results[1], results[3]))
    res = results[3]
    assert np.array_equal(res[1], images[1]) and res[1] is not images[1]
    for i in (0, 2, 3):
        assert np.array_equal(res[i], _one_after_another(images[i], masks[i], z[i], feather)), i
        keep = ref.feather_reference(masks[i], feather) == 0
        assert np.array_equal(res[i][keep], images[i][keep]) and not np.array_equal(res[i][masks[i] == 0], images[i][masks[i] == 0])
    # the single-window default is untouched by the new arguments, and differs where a window covers two groups
    one = inpaint.Inpainter(StandInG(), R, 'cpu', feather=feather, gather_fn=_gather_ref, paste_fn=lambda *a, **k: _paste_one(*a, **k))(images, masks, z=z)
    assert not np.array_equal(one[0], res[0]) and np.array_equal(one[3], res[3])
    # several samples: all windows of an image share its latents
    z3 = torch.from_numpy(rng.standard_normal((4, 2, 4)).astype(np.float32))
    res2 = inpaint.Inpainter(StandInG(), R, 'cpu', batch=2, **kw)(images, masks, z=z3, samples=2)
    for i in (0, 2, 3):
        for j in range(2):
            assert np.array_equal(res2[i][j], _one_after_another(images[i], masks[i], z3[i, j], feather)), (i, j)
    # more groups than max_windows: one window over all holes, as the default plans it
    inp = inpaint.Inpainter(StandInG(), R, 'cpu', batch=2, max_windows=2, **kw)
    few = inp(images, masks, z=z)
    assert [(i, k) for i, k, _, _ in inp.windows_] == [(0, 1), (2, 1), (2, 2), (3, 1)]
    assert inp.windows_[0][2] == inpaint.plan_window(masks[0], R, 0.5, feather) and np.array_equal(few[0], one[0]) and np.array_equal(few[2], res[2])
    for bad in (dict(windows='two'), dict(max_windows=256), dict(label_fn=hg.label_fn, owner_fn=None)):
        with pytest.raises(ValueError):
            inpaint.Inpainter(StandInG(), R, 'cpu', **{**kw, **bad})


def _paste_one(packed, packed_mask, shapes, windows, fake, k=1, feather=8):
    pk, pm, fake = packed.numpy(), packed_mask.numpy(), fake.numpy()
    out = np.stack([pk] * k)
    for n, ((h, w, off, moff), window) in enumerate(zip(shapes, windows)):
        for j in range(k):
            out[j, off:off + 3 * h * w] = ref.paste_reference(pk[off:off + 3 * h * w].reshape(h, w, 3), pm[moff:moff + h * w].reshape(h, w),
                                                              tuple(int(v) for v in window), fake[n * k + j], feather, np.float32)[0].reshape(-1)
    return torch.from_numpy(out)
