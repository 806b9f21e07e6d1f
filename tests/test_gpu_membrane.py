"""GPU: the gradient-domain paste-back (sh-gan_amd/inpaint.py ``paste_back_membrane`` on csrc/membrane.hip) against the float64 yardstick of
tests/membrane_f64.py: the solver alone (closed forms, conjugate gradients, determinism), the setup and the paste step alone, the whole
chain under the byte window, the identities with ``paste_back``, what the blend is for, refusals, the fill / guard runs of the new
allocation sites and ``Inpainter(blend='membrane')`` end to end.  Solver data is |d| <= 32; tol is the default 0.25 grey levels."""
import numpy as np
import pytest
import torch

import inpaint_f64 as ref
import membrane_f64 as mref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
R = 16
TOL = 0.25
_CACHE = {}


def _tc():
    from shgan_amd import inpaint
    return inpaint.MEMBRANE_TILE, inpaint.MEMBRANE_COARSEST


def _solve(problems, **kw):
    """problems: [(field float32 [h, w, 3], omega bool [h, w])] -> ([returned field per problem], info int [P, 3]): one ragged launch
    sequence, offsets that are no multiples of 4."""
    from shgan_amd import inpaint
    table, fo, oo = [], 0, 0
    for f, om in problems:
        h, w = om.shape
        table.append((h, w, fo, oo))
        fo, oo = fo + 3 * h * w + 1, oo + h * w + 3
    field = np.full(fo, 77.0, np.float32)
    omega = np.full(oo, 1, np.uint8)
    for (f, om), (h, w, a, b) in zip(problems, table):
        field[a:a + 3 * h * w] = np.asarray(f, np.float32).reshape(-1)
        omega[b:b + h * w] = np.asarray(om, np.uint8).reshape(-1) * 255           # (any non-zero byte is "unknown")
    fd, od = torch.from_numpy(field).to(DEV), torch.from_numpy(omega).to(DEV)
    info = inpaint.membrane_solve(fd, od, np.array(table), **kw)
    assert info.shape == (len(problems), 3) and info.dtype == torch.int32
    got = fd.cpu().numpy()
    gaps = np.ones(fo, bool)
    for h, w, a, b in table:
        gaps[a:a + 3 * h * w] = False
    assert np.all(got[gaps] == 77.0), 'a float between the problems changed'
    return [got[a:a + 3 * h * w].reshape(h, w, 3) for h, w, a, b in table], info.cpu().numpy()


def _norm(info_row):
    return float(np.array([info_row[1]], np.int32).view(np.float32)[0])


def _case(name, h, w, seed):
    key = ('solver', name, h, w, seed)
    if key not in _CACHE:
        om = mref.domain(name, h, w)
        f = mref.random_field(om, seed)
        _CACHE[key] = (f, om, mref.solve_reference(f, om))
    return _CACHE[key]


def _sizes():
    T, _ = _tc()
    return [(T - 1, T + 1), (T, T), (T + 1, T - 1), (2 * T + 3, T), (97, 2 * T + 3)]


# ------------------------------------------------------------------------------------------------
# the solver alone
# ------------------------------------------------------------------------------------------------

def test_solver_closed_forms():
    """Omega away from the grid edge with constant data -> the constant; data on a plane -> the plane (it is discrete-harmonic); both to
    tol, certified.  One pixel of Omega -> the mean of its four neighbours, to the
    rounding of its three additions (a few ulps of the data)."""
    probs, wants = [], []
    for h, w in _sizes():
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        for name in ('blob', 'inner'):
            om = mref.domain(name, h, w)
            for want in (np.full((h, w), -23.5), 0.21 * xx - 0.17 * yy + 3.0):
                want = np.stack([want, -want, 0.5 * want], axis=2)
                assert np.abs(want).max() <= 32
                probs.append((np.where(om[:, :, None], 0.0, want).astype(np.float32), om))
                wants.append(want)
    got, info = _solve(probs)
    assert np.all(info[:, 2] == 1), info
    for (f, om), g, want in zip(probs, got, wants):
        assert np.abs(g - want).max() <= TOL, (om.shape, np.abs(g - want).max())
    probs = []
    for i, (h, w) in enumerate(_sizes() + [(5, 7)]):
        om = np.zeros((h, w), bool)
        om[h // 2, w // 3] = True
        probs.append((mref.random_field(om, 50 + i), om))
    got, info = _solve(probs)
    assert np.all(info[:, 2] == 1), info
    for (f, om), g in zip(probs, got):
        (y,), (x,) = np.nonzero(om.any(axis=1)), np.nonzero(om.any(axis=0))
        nb = np.stack([f[y - 1, x], f[y + 1, x], f[y, x - 1], f[y, x + 1]]).astype(np.float64)
        want = nb.sum(axis=0) / 4
        # three float32 additions of partial sums no larger than S = sum |neighbour|, then an exact quarter: 0.75 S 2^-24
        assert np.all(np.abs(g[y, x] - want) <= 0.75 * 2.0 ** -24 * np.abs(nb).sum(axis=0)), (om.shape, g[y, x], want)
        assert np.array_equal(g[~om], f[~om])


def _solver_case_ids():
    return [f'{n}-{h}x{w}' for n, h, w, _ in mref.solver_cases(32, 16)]


@pytest.mark.parametrize('idx', range(len(mref.solver_cases(32, 16))), ids=_solver_case_ids())
def test_solver_against_the_yardstick(idx):
    """Certified at the default cycle budget; the float64 residual of the returned field, through the bound, certifies tol on its own; the
    distance to the conjugate-gradient solution is within tol; nothing outside Omega changes by a bit."""
    T, C = _tc()
    name, h, w, seed = mref.solver_cases(T, C)[idx]
    f, om, c64 = _case(name, h, w, seed)
    (got,), info = _solve([(f, om)])
    n = mref.omega_box_side(om)
    r64 = mref.residual_f64(got, om)
    err = float(np.abs(got - c64).max())
    print(f'{name} {h}x{w}: n = {n}, cycles {info[0, 0]}, state {info[0, 2]}, device norm {_norm(info[0]):.3e}, float64 residual {r64:.3e} '
          f'(bound {r64 * (n + 1) ** 2 / 8:.3e}), |c - c64| = {err:.3e}')
    assert info[0, 2] == 1, info
    assert r64 * (n + 1) ** 2 / 8 <= TOL
    assert err <= TOL + 1e-6
    assert np.array_equal(got[~om].view(np.int32), f[~om].view(np.int32))


def test_solver_states_and_budget():
    """max_cycles = 0 leaves the field alone and reports state 0 with the first norm; a tolerance float32 cannot reach ends in state 2
    with a norm at the float32 floor, and the field is still the solution to far better than tol."""
    f, om, c64 = _case('blob', 97, 67, 40)
    (got,), info0 = _solve([(f, om)], max_cycles=0)
    assert info0[0].tolist()[::2] == [0, 0] and np.array_equal(got, f) and _norm(info0[0]) > 1.0
    (got,), info = _solve([(f, om)], tol=1e-9)
    assert info[0, 2] == 2 and 0 < info[0, 0] < 40 and _norm(info[0]) < 1e-4, (info, _norm(info[0]))
    assert np.abs(got - c64).max() <= 0.01
    (got1,), info1 = _solve([(f, om)], max_cycles=1)
    assert info1[0].tolist()[::2] == [1, 0] and _norm(info1[0]) < 0.5 * _norm(info0[0]) and not np.array_equal(got1, f)


def test_solver_is_deterministic_and_independent_of_the_batch():
    T, C = _tc()
    a, b, c = _case('corridor', 97, 2 * T + 3, 33), _case('blob', T + 1, T - 1, 20), _case('edge', C - 2, C, 91)
    batch = [(a[0], a[1]), (b[0], b[1]), (c[0], c[1])]
    got1, info1 = _solve(batch)
    got2, info2 = _solve(batch)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(got1, got2)) and np.array_equal(info1, info2)
    for i, prob in enumerate(batch):
        (alone,), info = _solve([prob])
        assert np.array_equal(alone.view(np.int32), got1[i].view(np.int32)) and np.array_equal(info[0], info1[i]), i
    # two samples that share one Omega = two separate solves
    from shgan_amd import inpaint
    f0, om, _ = a
    f1 = mref.random_field(om, 34)
    h, w = om.shape
    field = torch.from_numpy(np.concatenate([f0.reshape(-1), f1.reshape(-1)])).to(DEV)
    omega = torch.from_numpy(om.astype(np.uint8).reshape(-1)).to(DEV)
    info = inpaint.membrane_solve(field, omega, np.array([[h, w, 0, 0], [h, w, 3 * h * w, 0]]))
    both = field.cpu().numpy().reshape(2, h, w, 3)
    (s1,), i1 = _solve([(f1, om)])
    assert np.array_equal(both[0].view(np.int32), got1[0].view(np.int32)) and np.array_equal(both[1].view(np.int32), s1.view(np.int32))
    assert np.array_equal(info.cpu().numpy(), np.stack([info1[0], i1[0]]))


# ------------------------------------------------------------------------------------------------
# images
# ------------------------------------------------------------------------------------------------

ALL = tuple(range(len(ref.CASES)))


def _batch(ids, k=1):
    key = ('batch', tuple(ids), k)
    if key not in _CACHE:
        from shgan_amd import inpaint, resize
        cases = [ref.make_case(i, R, k) for i in ids]
        packed, shapes = resize.pack_images([c[0] for c in cases])
        packed_mask, moffs = inpaint.pack_masks([c[1] for c in cases])
        shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
        windows = np.array([c[2] for c in cases], np.int64)
        fake = torch.from_numpy(np.concatenate([c[3] for c in cases]))
        boxes = np.array([ref.hole_box(c[1]) for c in cases], np.int64)
        _CACHE[key] = (cases, packed, packed_mask, shapes, windows, fake, boxes)
    cases, packed, packed_mask, shapes, windows, fake, boxes = _CACHE[key]
    return cases, packed.to(DEV), packed_mask.to(DEV), shapes, windows, fake.to(DEV), boxes


def _images(out, shapes):
    out = out.cpu().numpy()
    return [[row[off:off + 3 * h * w].reshape(h, w, 3) for h, w, off in shapes[:, :3]] for row in out]


def _chain64(idx, feather, j):
    """The float64 chain of case idx, sample j (of the k = 3 draw; sample 0 is the k = 1 draw), cached."""
    key = ('chain', idx, feather, j)
    if key not in _CACHE:
        img, m, window, fake = ref.make_case(idx, R, 3)
        for jj in range(3):
            _CACHE[('chain', idx, feather, jj)] = mref.paste_reference(img, m, window, fake[jj], feather)
    return _CACHE[key]


def _run_setup(boxes_on, k=1, feather=5):
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, fake, boxes = _batch(ALL, k)
    plan = inpaint.membrane_plan(shapes, windows, feather, k, boxes if boxes_on else None)
    g = torch.full((plan.g_elems,), float('nan'), device=DEV)
    field = torch.full((plan.g_elems,), float('nan'), device=DEV)
    omega = torch.full((plan.omega_bytes,), 7, dtype=torch.uint8, device=DEV)
    inpaint.membrane_setup(packed, pm, shapes, windows, fake, plan, g, field, omega, feather)
    return cases, plan, g.cpu().numpy(), field.cpu().numpy(), omega.cpu().numpy()


@pytest.mark.parametrize('boxes_on', (False, True))
def test_setup_equals_the_restatement(boxes_on):
    """g within ``eps_of`` of the float64 resample chain; Omega exactly {A > 0}; the field exactly float32(orig - g) of the device's own g
    where A = 0 and 0 in Omega; with the holes' boxes the same values on the smaller grid."""
    k, feather = 2, 5
    cases, plan, g, field, omega = _run_setup(boxes_on, k, feather)
    for i, (img, m, window, fake) in enumerate(cases):
        y0, x0, ch, cw = window
        gy0, gx0, gh, gw, foff, ooff = (int(v) for v in plan.grids[i])
        if not boxes_on:
            assert (gy0, gx0, gh, gw) == (0, 0, ch, cw)
        eps = ref.eps_of(R, ch, cw)
        om = omega[ooff:ooff + gh * gw].reshape(gh, gw)
        for j in range(k):
            g64, f64, om64, A = mref.setup_reference(img, m, window, fake[j], feather)
            sl = (slice(gy0, gy0 + gh), slice(gx0, gx0 + gw))
            assert np.array_equal(om, om64[sl].astype(np.uint8)), i
            assert om64.sum() == om.sum()                                       # Omega lies inside the grid
            a = foff + j * 3 * gh * gw
            gd, fd = g[a:a + 3 * gh * gw].reshape(gh, gw, 3), field[a:a + 3 * gh * gw].reshape(gh, gw, 3)
            assert np.abs(gd - g64[sl]).max() <= eps, (i, j)
            orig = img[y0:y0 + ch, x0:x0 + cw][sl].astype(np.float32)
            want = np.where(om64[sl][:, :, None], np.float32(0), orig - gd)
            assert np.array_equal(fd.view(np.int32), want.view(np.int32)), (i, j)


def test_setup_g_is_the_bits_paste_back_blends():
    """feather = 0, a hole-filled window: A = 1 everywhere, paste_back stores (uint8)(int)g.  The same bytes come out of the membrane
    paste fed setup's g and c = 0."""
    from shgan_amd import inpaint
    (case,), packed, pm, shapes, windows, fake, boxes = _batch((10,))
    want = inpaint.paste_back(packed, pm, shapes, windows, fake, feather=0)
    plan = inpaint.membrane_plan(shapes, windows, 0, 1)
    g = torch.full((plan.g_elems,), float('nan'), device=DEV)
    field, omega = torch.full_like(g, float('nan')), torch.full((plan.omega_bytes,), 7, dtype=torch.uint8, device=DEV)
    inpaint.membrane_setup(packed, pm, shapes, windows, fake, plan, g, field, omega, 0)
    assert bool((field[:3 * 41 * 23] == 0).all()) and bool((omega[:41 * 23] == 1).all())       # (the buffers are rounded up to 16 bytes)
    out = packed.clone().view(1, -1)
    inpaint.membrane_paste(pm, shapes, windows, plan, g, field, out, R, 0)
    assert torch.equal(out, want)
    gi = g.cpu().numpy()[:3 * 41 * 23].reshape(41, 23, 3)
    assert np.array_equal(gi.astype(np.int64).astype(np.uint8), want.cpu().numpy().reshape(41, 23, 3))


def _sharp_rule(got, img, window, t, A, u64, eps):
    """The byte rule of inpaint_f64 for a membrane paste: at most 1 off, equal where A = 0, equal wherever t is farther than eps from an
    integer (a value clamped in both precisions is exact in both) -> share of window pixels left out."""
    y0, x0, ch, cw = window
    g = got[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
    w = np.where(A[:, :, None] > 0, t.astype(np.int64), img[y0:y0 + ch, x0:x0 + cw].astype(np.int64))
    outside = np.ones(got.shape[:2], bool)
    outside[y0:y0 + ch, x0:x0 + cw] = False
    assert np.array_equal(got[outside], img[outside])
    assert np.abs(g - w).max() <= 1
    assert np.array_equal(g[A == 0], w[A == 0])
    clamped = (u64 <= -eps) | (u64 >= 255.0 + eps)
    near = (np.abs(t - np.rint(t)) <= eps) & (A[:, :, None] > 0) & ~clamped
    assert np.array_equal(g[~near], w[~near]), f'{int((g != w)[~near].sum())} bytes differ farther than {eps:.3e} from an integer'
    return float(near.any(axis=2).sum()) / (ch * cw)


# (case, feather) whose float64 restatement alone puts more than 1 % of the window within eps of an integer, so the share says nothing
# about the device there: the 19 x 21 window of case 11 at feather 32 has 4 such pixels of 399 (1.003 %); every other pair stays under
# 0.71 %.  The bytes of such a pair are held to the rule all the same.
SHARE_LEFT_OUT = {(11, 32)}


@pytest.mark.parametrize('feather', (0, 5, 32))
def test_paste_alone_obeys_the_sharp_byte_rule(feather):
    """The paste step fed the float32-rounded yardstick membrane: g + c differs from float64 by g's eps, c's rounding and one addition
    (eps + 2^-20 255 in all), so the bytes obey the sharp rule of ``paste_back``; at most 1 % of a window lies that near an integer."""
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, fake, boxes = _batch(ALL)
    plan = inpaint.membrane_plan(shapes, windows, feather, 1, boxes)
    g = torch.full((plan.g_elems,), float('nan'), device=DEV)
    field, omega = torch.full_like(g, float('nan')), torch.full((plan.omega_bytes,), 7, dtype=torch.uint8, device=DEV)
    inpaint.membrane_setup(packed, pm, shapes, windows, fake, plan, g, field, omega, feather)
    fh = field.cpu().numpy()
    refs = []
    for i, (img, m, window, f) in enumerate(cases):
        want, t, A, c64 = _chain64(i, feather, 0)
        gy0, gx0, gh, gw, foff, ooff = (int(v) for v in plan.grids[i])
        fh[foff:foff + 3 * gh * gw] = c64[gy0:gy0 + gh, gx0:gx0 + gw].astype(np.float32).reshape(-1)
        refs.append((t, A, c64))
    out = packed.clone().view(1, -1)
    alpha = torch.full((pm.numel(),), 9, dtype=torch.uint8, device=DEV)
    inpaint.membrane_paste(pm, shapes, windows, plan, g, torch.from_numpy(fh).to(DEV), out, R, feather, alpha_out=alpha)
    got, alpha = _images(out, shapes)[0], alpha.cpu().numpy()
    worst = 0.0
    for i, (img, m, window, f) in enumerate(cases):
        t, A, c64 = refs[i]
        y0, x0, ch, cw = window
        g64 = mref.setup_reference(img, m, window, f[0], feather)[0]
        share = _sharp_rule(got[i], img, window, t, A, g64 + c64, ref.eps_of(R, ch, cw) + 2.0 ** -20 * 255)
        if (i, feather) not in SHARE_LEFT_OUT:
            assert share <= ref.CAP, (i, share)
            worst = max(worst, share)
        h, w, _, moff = shapes[i]
        wa = np.zeros((h, w), np.uint8)
        wa[y0:y0 + ch, x0:x0 + cw] = A
        assert np.array_equal(alpha[moff:moff + h * w].reshape(h, w), wa)
    print(f'feather {feather}: at most {worst:.4%} of a window within eps of an integer')


@pytest.mark.parametrize('k', (1, 3))
@pytest.mark.parametrize('feather', (0, 5, 32))
def test_whole_chain_lies_in_the_byte_window(k, feather):
    """The twelve shapes of ``inpaint_f64.make_case``, one ragged call: every byte in byte_window(v64, eps + tol), every byte with A = 0
    the original's; every problem ends certified or at the float32 floor."""
    from shgan_amd import inpaint
    cases, packed, pm, shapes, windows, fake, boxes = _batch(ALL, k)
    info = torch.full((len(cases) * k, 3), -5, dtype=torch.int32, device=DEV)
    out = inpaint.paste_back_membrane(packed, pm, shapes, windows, fake, k=k, feather=feather, info_out=info, boxes=boxes if k == 3 else None)
    assert out.shape == (k, packed.numel()) and out.dtype == torch.uint8
    got, info = _images(out, shapes), info.cpu().numpy()
    print(f'k = {k}, feather = {feather}: states {np.bincount(info[:, 2], minlength=3).tolist()}, cycles up to {info[:, 0].max()}')
    assert np.all((info[:, 2] == 1) | (info[:, 2] == 2)), info
    for i, (img, m, window, f) in enumerate(cases):
        y0, x0, ch, cw = window
        for j in range(k):
            want, t, A, c64 = _chain64(i, feather, j)
            lo, hi = mref.byte_window(t, ref.eps_of(R, ch, cw) + TOL)
            gw_ = got[j][i][y0:y0 + ch, x0:x0 + cw].astype(np.int64)
            inside = A[:, :, None] > 0
            assert np.all((gw_ >= lo) & (gw_ <= hi) | ~inside), (i, j, int(((gw_ < lo) | (gw_ > hi))[np.broadcast_to(inside, gw_.shape)].sum()))
            keep = np.ones(img.shape[:2], bool)
            keep[y0:y0 + ch, x0:x0 + cw] = A == 0
            assert np.array_equal(got[j][i][keep], img[keep]), (i, j)


def test_identities_with_paste_back():
    """A window filled by its hole: no Dirichlet data, c = 0, paste_back's bytes.  An original that equals g on every window pixel with
    A = 0: d = 0, c = 0, paste_back's bytes."""
    from shgan_amd import inpaint, resize
    for feather in (0, 5, 32):
        _, packed, pm, shapes, windows, fake, boxes = _batch((10,), 2)
        info = torch.full((2, 3), -5, dtype=torch.int32, device=DEV)
        a = inpaint.paste_back_membrane(packed, pm, shapes, windows, fake, k=2, feather=feather, info_out=info)
        assert torch.equal(a, inpaint.paste_back(packed, pm, shapes, windows, fake, k=2, feather=feather))
        assert info.cpu().numpy().tolist() == [[0, 0, 1]] * 2                  # certified before the first cycle, norm 0
    rng = np.random.RandomState(3)
    img = np.full((60, 75, 3), 128, np.uint8)
    mask = ref.mask_with_holes(60, 75, [(20, 41, 30, 52), (5, 6, 70, 71)])
    img[mask == 0] = rng.randint(0, 256, (int((mask == 0).sum()), 3))
    window = (2, 10, 55, 65)
    img[:2] = rng.randint(0, 256, (2, 75, 3))                                  # (outside the window anything goes)
    fake = torch.full((1, 3, R, R), 1.0 / 255.0)                               # g = 128 exactly: 0.5 + 127.5 absorbs the resample's last bits
    packed, shapes = resize.pack_images([img])
    pm, moffs = inpaint.pack_masks([mask])
    shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
    for feather in (0, 4):
        args = (packed.to(DEV), pm.to(DEV), shapes, np.array([window]), fake.to(DEV))
        a = inpaint.paste_back_membrane(*args, feather=feather, boxes=np.array([ref.hole_box(mask)]))
        b = inpaint.paste_back(*args, feather=feather)
        assert torch.equal(a, b) and not torch.equal(a.cpu()[0], packed)


def test_the_blend_removes_an_offset_the_feather_leaves():
    """A smooth original and a generator output equal to it plus 12 grey levels (R x R window: the resample is the identity).  The
    membrane takes the offset out: within 1 of the original everywhere.  The feather alone leaves it: at least 6 off inside the hole."""
    from shgan_amd import inpaint, resize
    n = 64
    yy, xx = np.mgrid[0:n, 0:n]
    img = np.stack([60 + xx + yy // 2 + 10 * c for c in range(3)], axis=2).astype(np.uint8)
    mask = ref.mask_with_holes(n, n, [(18, 47, 15, 44)])
    fake = torch.from_numpy(((img.astype(np.float64) + 12.0 - 127.5) / 127.5).astype(np.float32).transpose(2, 0, 1)[None].copy())
    packed, shapes = resize.pack_images([img])
    pm, moffs = inpaint.pack_masks([mask])
    shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
    args = (packed.to(DEV), pm.to(DEV), shapes, np.array([[0, 0, n, n]]), fake.to(DEV))
    info = torch.full((1, 3), -5, dtype=torch.int32, device=DEV)
    mem = inpaint.paste_back_membrane(*args, feather=8, info_out=info).cpu().numpy().reshape(n, n, 3).astype(np.int64)
    fea = inpaint.paste_back(*args, feather=8).cpu().numpy().reshape(n, n, 3).astype(np.int64)
    assert info.cpu().numpy()[0, 2] == 1
    assert np.abs(mem - img).max() <= 1
    assert np.abs(fea - img)[mask == 0].max() >= 6


def test_refusals():
    from shgan_amd import _lib, inpaint
    _, packed, pm, shapes, windows, fake, boxes = _batch((1,))
    ok = inpaint.paste_back_membrane(packed, pm, shapes, windows, fake)
    n = packed.numel()
    for kw in (dict(packed=packed.cpu()), dict(fake=fake.cpu()), dict(fake=fake.double()), dict(fake=fake[:, :2]), dict(packed=packed.float()),
               dict(feather=33), dict(k=2), dict(out=torch.zeros(2, n, dtype=torch.uint8, device=DEV)), dict(out=torch.zeros(1, n, device=DEV)),
               dict(info_out=torch.zeros(2, 3, dtype=torch.int32, device=DEV)), dict(info_out=torch.zeros(1, 3, device=DEV)), dict(tol=0.0)):
        a = dict(packed=packed, packed_mask=pm, shapes=shapes, windows=windows, fake=fake)
        a.update(kw)
        with pytest.raises(_lib.ShgError):
            inpaint.paste_back_membrane(**a)
    both = torch.zeros(2 * n, dtype=torch.uint8, device=DEV)
    both[:n] = packed
    with pytest.raises(_lib.ShgError, match='overlaps'):
        inpaint.paste_back_membrane(both[:n], pm, shapes, windows, fake, out=both[n // 2:n // 2 + n].view(1, n))
    f = torch.zeros(3 * 20 * 20, device=DEV)
    om = torch.ones(20 * 20, dtype=torch.uint8, device=DEV)
    table = np.array([[20, 20, 0, 0]])
    with pytest.raises(_lib.ShgError, match='workspace|ws'):
        inpaint.membrane_solve(f, om, table, ws=torch.zeros(inpaint.membrane_workspace_bytes(1, 20, 20) - 1, dtype=torch.uint8, device=DEV))
    for bad in (dict(field=f[:-1]), dict(field=f.cpu()), dict(field=f.double()), dict(omega=om[:-1]), dict(omega=om.float()),
                dict(table=np.array([[20, 20, 0, 0], [20, 20, 600, 0]])), dict(table=np.array([[0, 20, 0, 0]])), dict(max_cycles=-1), dict(n=np.array([0]))):
        a = dict(field=f, omega=om, table=table)
        a.update(bad)
        with pytest.raises(_lib.ShgError):
            inpaint.membrane_solve(**a)
    assert torch.equal(ok, inpaint.paste_back_membrane(packed, pm, shapes, windows, fake))          # (a refusal leaves nothing behind)


def test_new_sites_do_not_depend_on_fresh_contents_and_stay_inside_their_buffers():
    """('inpaint.py', 'paste_back_membrane') -- g, the field, Omega, the solver's workspace, the result -- and ('inpaint.py',
    'membrane_solve') -- the workspace and info when the caller gives none: the same bits with every fresh allocation pre-filled with NaN
    bytes and with large values, and no guard band touched with every buffer housed between poisoned bands.  The workspaces are the
    point: the shadow, the coarse levels and the partial maxima are written before they are read."""
    import alloc_fill
    import alloc_guard
    from shgan_amd import inpaint
    sites = {('inpaint.py', 'paste_back_membrane'), ('inpaint.py', 'membrane_solve')}
    ids = (1, 4, 6, 11, 8)
    cases, _, _, shapes, windows, _, boxes = _batch(ids, 2)
    host = _CACHE[('batch', ids, 2)]
    f, om, _ = _case('corridor', 97, 67, 33)
    h, w = om.shape

    def run():
        packed, pm, fake = host[1].to(DEV), host[2].to(DEV), host[5].to(DEV)
        alpha = torch.empty(pm.numel(), dtype=torch.uint8, device=DEV)
        info = torch.empty(len(ids) * 2, 3, dtype=torch.int32, device=DEV)
        out = inpaint.paste_back_membrane(packed, pm, shapes, windows, fake, k=2, feather=5, alpha_out=alpha, info_out=info, boxes=boxes)
        field, omega = torch.from_numpy(f.reshape(-1)).to(DEV), torch.from_numpy(om.astype(np.uint8).reshape(-1)).to(DEV)
        info2 = inpaint.membrane_solve(field, omega, np.array([[h, w, 0, 0]]))
        return [out, alpha, info, field, info2]
    want = run()
    torch.cuda.synchronize()
    for pattern in ('nan', 'big'):
        with alloc_fill.filled(pattern) as rec:
            got = run()
            torch.cuda.synchronize()
        assert sites <= rec.sites, rec.sites
        assert all(torch.equal(x, y) for x, y in zip(got, want)), pattern
    with alloc_guard.guarded() as rec:
        got = run()
        bad = rec.violations()
        assert sites <= rec.sites and not bad, bad
        assert all(torch.equal(x, y) for x, y in zip(got, want))


@pytest.fixture(scope='module')
def small_g():
    from shgan_amd import configs
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1)
    return G.eval().requires_grad_(False).to(DEV)


def test_inpainter_membrane_end_to_end(small_g):
    """The reduced-width seeded generator at R = 256, two photographs of different sizes, two samples: away from Omega the bytes are the
    originals, inside the hole they are not, and every problem ends certified or at the float32 floor.  (The random weights
    saturate, so two samples of a small hole may clamp to the same bytes: the samples are not compared.)"""
    from shgan_amd import inpaint
    rng = np.random.RandomState(7)
    sizes = [(300, 420), (481, 333)]
    images = [ref.random_image(rng, h, w) for h, w in sizes]
    masks = [ref.mask_with_holes(300, 420, [(100, 180, 150, 260)]), ref.mask_with_holes(481, 333, [(200, 230, 100, 120), (260, 262, 140, 141)])]
    z = torch.from_numpy(rng.standard_normal((2, 2, 64)).astype(np.float32))
    inp = inpaint.Inpainter(small_g, 256, DEV, feather=8, blend='membrane')
    res = inp(images, masks, z=z, samples=2)
    assert [r.shape for r in res] == [(2,) + im.shape for im in images]
    assert len(inp.info) == 1 and inp.info[0].shape == (4, 3) and np.all((inp.info[0][:, 2] == 1) | (inp.info[0][:, 2] == 2)), inp.info
    print('info', inp.info[0].tolist())
    for i, (img, m) in enumerate(zip(images, masks)):
        y0, x0, ch, cw = inpaint.plan_window(m, 256, 0.5, 8)
        A = ref.feather_reference(m[y0:y0 + ch, x0:x0 + cw], 8)
        keep = np.ones(img.shape[:2], bool)
        keep[y0:y0 + ch, x0:x0 + cw] = A == 0
        for j in range(2):
            assert np.array_equal(res[i][j][keep], img[keep]) and not np.array_equal(res[i][j][m == 0], img[m == 0])
