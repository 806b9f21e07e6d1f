"""GPU: the hole groups of sh-gan_amd/inpaint.py (``label_holes`` / ``fetch_components`` / ``owner_plane`` on csrc/hole_label.hip) against
the numpy yardstick of tests/hole_groups_ref.py, bit for bit; the keyed paste-backs against the UNKEYED kernels applied once per group
with that group's mask (the yardstick is the parent's kernel, not the new one); refusals; the fill / guard runs of the new allocation
sites; ``Inpainter(windows='per_hole')`` end to end.  INTEGRATION section T states the definitions."""
import numpy as np
import pytest
import torch

import hole_groups_ref as hg
import inpaint_f64 as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
R = 16
_CACHE = {}


def _T():
    from shgan_amd import inpaint
    return inpaint.hole_label_tile()


def _want(masks, feather):
    key = ('want', tuple((m.shape, m.tobytes()) for m in masks), feather)
    if key not in _CACHE:
        _CACHE[key] = hg.pack_reference(masks, feather)
    return _CACHE[key]


def _label(masks, feather, cap=4096):
    """-> (HoleLabels, packed mask on the device, shapes [B, 4], labels as numpy, state row 0 as numpy)."""
    from shgan_amd import inpaint
    pm, moffs = inpaint.pack_masks(masks)
    shapes = np.array([(m.shape[0], m.shape[1], 3 * o, o) for m, o in zip(masks, moffs)], np.int64)
    pm = pm.to(DEV)
    lbl = inpaint.label_holes(pm, shapes, feather, max_components=cap)
    assert lbl.labels.dtype == torch.int32 and lbl.labels.shape == (pm.numel(),)
    return lbl, pm, shapes, lbl.labels.cpu().numpy(), lbl.state[0].cpu().numpy()


def _keys_of(comps):
    """(image, root) -> key: 1, 2, ... by increasing root within the image (wrapped into 1..255)."""
    table, seen = [], {}
    for im, root in comps[:, :2]:
        seen[im] = seen.get(im, 0) + 1
        table.append((im, root, (seen[im] - 1) % 255 + 1))
    return np.array(table, np.int64).reshape(-1, 3)


def _check(masks, feather, name):
    """Labels, components and owner plane of one launch sequence equal the reference, bit for bit; no loop cap was hit."""
    from shgan_amd import inpaint
    want_labels, want_comps = _want(masks, feather)
    lbl, pm, shapes, labels, head = _label(masks, feather)
    assert head[1] == 0, (name, 'flags', head[:2])
    assert head[0] == want_comps.shape[0], (name, head[:2])
    assert np.array_equal(labels, want_labels), (name, int((labels != want_labels).sum()))
    comps = inpaint.fetch_components(lbl)
    assert comps.dtype == np.int64 and np.array_equal(comps, want_comps), (name, comps, want_comps)
    table = _keys_of(want_comps)
    owner = inpaint.owner_plane(lbl, pm, shapes, table).cpu().numpy()
    off = 0
    for i, m in enumerate(masks):
        n = m.size
        keys = {int(r): int(k) for im, r, k in table if im == i}
        want = hg.owner_reference(m, want_labels[off:off + n].reshape(m.shape), keys)
        assert np.array_equal(owner[off:off + n].reshape(m.shape), want), (name, i)
        off += n
    return labels, comps, owner


@pytest.mark.parametrize('feather', (0, 3))
def test_single_images_equal_the_reference(feather):
    """Sizes 5 x 7, T x T, (T + 1) x (T - 1), (2T + 3) x (3T + 1), each empty / all hole / the four corner pixels / random specks; the
    gap of 2r and 2r + 1 known pixels along a row, a column and both diagonals across a tile seam and the four-tile corner; D touching only
    diagonally across the corner; the comb and the spiral over 2 x 2 tiles (the longest label chains: the cap flag must stay clear, which
    ``_check`` asserts for every case); column w - 1 against column 0 of the next row."""
    T, r = _T(), feather + 1
    for name, m in hg.single_cases(T, r):
        labels, comps, owner = _check([m], feather, name)
        h, w = m.shape
        if name.startswith('empty'):
            assert comps.shape == (0, 7) and np.all(labels == -1) and not owner.any()
        if name.startswith('all'):
            assert comps.tolist() == [[0, 0, 0, h, 0, w, h * w]] and not labels.any() and np.all(owner == 1)
        if name.startswith('corners') and min(h, w) > 4 * r + 2:
            assert comps[:, 1:].tolist() == [[0, 0, 1, 0, 1, 1], [w - 1 - r, 0, 1, w - 1, w, 1], [(h - 1 - r) * w, h - 1, h, 0, 1, 1],
                                             [(h - 1 - r) * w + w - 1 - r, h - 1, h, w - 1, w, 1]]
        if name in ('comb', 'spiral', 'dtouch-diag', 'dtouch-anti'):
            assert comps.shape[0] == 1, name
        if name == 'wrap':
            assert comps.shape[0] == 2
    for name, m, groups in hg.gap_cases(T, r):
        assert _want([m], feather)[1].shape[0] == groups, name          # (the device's count was held to the reference's above)


@pytest.mark.parametrize('feather', (0, 3))
def test_a_ragged_pack_equals_each_image_alone_and_itself(feather):
    """Five images of different sizes in one launch sequence: a hole in the last row of image i above one in the first row of image i + 1
    stay apart; every image's labels and components are those of the image labelled alone; a second run gives the same bits."""
    from shgan_amd import inpaint
    T, r = _T(), feather + 1
    masks = hg.pack_case(T, r)
    labels, comps, owner = _check(masks, feather, 'pack')
    assert (comps[:, 0] == 0).sum() == 1 and (comps[:, 0] == 1).sum() == 2
    labels2, comps2, owner2 = _check(masks, feather, 'pack again')
    assert np.array_equal(labels, labels2) and np.array_equal(comps, comps2) and np.array_equal(owner, owner2)
    off = 0
    for i, m in enumerate(masks):
        lbl, pm, shapes, alone, head = _label([m], feather)
        assert np.array_equal(alone, labels[off:off + m.size]), i
        c = inpaint.fetch_components(lbl)
        c[:, 0] = i
        assert np.array_equal(c, comps[comps[:, 0] == i]), i
        off += m.size


def test_capacity():
    """Five groups into a capacity of two: flag bit 0, the count still five, the labels complete, two rows of comps are real groups, and
    ``fetch_components`` raises naming the capacity."""
    from shgan_amd import inpaint
    T = _T()
    m = np.ones((T + 9, 2 * T + 5), np.uint8)
    for y, x in ((2, 2), (2, 2 * T), (T + 6, 3), (T + 5, 2 * T + 2), (T // 2, T)):
        m[y, x] = 0
    want_labels, want_comps = _want([m], 3)
    assert want_comps.shape[0] == 5
    lbl, pm, shapes, labels, head = _label([m], 3, cap=2)
    assert head[0] == 5 and head[1] == 1
    assert np.array_equal(labels, want_labels)
    rows = lbl.state[1:].cpu().numpy().astype(np.int64)
    assert rows.shape == (2, 8) and all(any(np.array_equal(r[:7], c) for c in want_comps) for r in rows) and not np.array_equal(rows[0], rows[1])
    with pytest.raises(ValueError, match='max_components = 2'):
        inpaint.fetch_components(lbl)


# ------------------------------------------------------------------------------------------------
# keyed paste-back
# ------------------------------------------------------------------------------------------------

# image 0, 100 x 140, three groups at feather 5 (r = 6): the 40 x 40 hole's window [10:90, 10:90] covers the 2 x 2 hole at columns 83..84
# entirely -- its ring reaches column 89 -- while 13 known columns (70..82) keep the two apart; image 1, 64 x 90, two groups
HOLES = [(100, 140, [(30, 70, 30, 70), (45, 47, 83, 85), (90, 93, 120, 130)]), (64, 90, [(5, 15, 5, 20), (40, 50, 60, 80)])]


def _paste_case(k, feather):
    key = ('paste', k, feather)
    if key not in _CACHE:
        from shgan_amd import inpaint, resize
        rng = np.random.RandomState(40 + k)
        images = [ref.random_image(rng, h, w) for h, w, _ in HOLES]
        masks = [ref.mask_with_holes(h, w, boxes) for h, w, boxes in HOLES]
        packed, shapes = resize.pack_images(images)
        pm, moffs = inpaint.pack_masks(masks)
        shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
        comps = hg.pack_reference(masks, feather)[1]
        assert [(comps[:, 0] == i).sum() for i in range(2)] == [3, 2]
        plan = inpaint.plan_windows(comps, shapes, R, 0.5, feather)
        assert plan.image.tolist() == [0, 0, 0, 1, 1] and plan.key.tolist() == [1, 2, 3, 1, 2]
        if feather == 5:
            y0, x0, ch, cw = plan.windows[0]
            assert (y0, x0, ch, cw) == (10, 10, 80, 80) and x0 + cw >= 85 + feather                     # window 0 covers group 2 and its ring
        fake = torch.from_numpy(rng.uniform(-0.6, 0.6, (5 * k, 3, R, R)).astype(np.float32))
        groups = [gm for m in masks for _, gm in hg.group_masks(m, feather)]                            # in (image, root) = window order
        _CACHE[key] = (images, masks, packed, pm, shapes, plan, fake, groups)
    return _CACHE[key]


def _owner_of(masks, shapes, plan, feather):
    from shgan_amd import inpaint
    pm = inpaint.pack_masks(masks)[0].to(DEV)
    lbl = inpaint.label_holes(pm, shapes, feather)
    assert np.array_equal(inpaint.fetch_components(lbl)[:, :2], plan.table[:, :2])
    return inpaint.owner_plane(lbl, pm, shapes, plan.table)


def _per_group(fn, k, feather, **kw):
    """The unkeyed ``fn`` (``paste_back`` / ``paste_back_membrane``) once per window on that group's own mask -> (expected out [k, bytes],
    expected alpha plane, the per-window extras)."""
    from shgan_amd import inpaint
    images, masks, packed, pm, shapes, plan, fake, groups = _paste_case(k, feather)
    pk = packed.to(DEV)
    want, alpha_sum, extras = packed.numpy()[None].repeat(k, 0).copy(), np.zeros(pm.numel(), np.int64), []
    for n, (i, window, gm) in enumerate(zip(plan.image, plan.windows, groups)):
        h, w, off, moff = shapes[i]
        own = [gm if j == i else np.ones_like(m) for j, m in enumerate(masks)]
        gpm = inpaint.pack_masks(own)[0].to(DEV)
        alpha = torch.full((pm.numel(),), 9, dtype=torch.uint8, device=DEV)
        extra = {key: make(n) for key, make in kw.items()}
        out = fn(pk, gpm, shapes[i:i + 1], window[None], fake[n * k:(n + 1) * k].to(DEV), k=k, feather=feather, alpha_out=alpha, **extra).cpu().numpy()
        extras.append(extra)
        alpha = alpha.cpu().numpy()
        ring = alpha[moff:moff + h * w].reshape(h, w) > 0
        for j in range(k):
            want[j, off:off + 3 * h * w].reshape(h, w, 3)[ring] = out[j, off:off + 3 * h * w].reshape(h, w, 3)[ring]
        assert not np.any(alpha_sum[alpha > 0])                                                         # the rings are disjoint
        alpha_sum += alpha
    return want, alpha_sum.astype(np.uint8), extras


def _whole_alpha(masks, feather):
    return np.concatenate([ref.feather_reference(m, feather).reshape(-1) for m in masks])


@pytest.mark.parametrize('k', (1, 2))
@pytest.mark.parametrize('feather', (0, 5))
def test_keyed_paste_equals_the_unkeyed_kernel_once_per_group(k, feather):
    from shgan_amd import inpaint
    images, masks, packed, pm, shapes, plan, fake, groups = _paste_case(k, feather)
    want, want_alpha, _ = _per_group(inpaint.paste_back, k, feather)
    owner = _owner_of(masks, shapes, plan, feather)
    alpha = torch.full((pm.numel(),), 9, dtype=torch.uint8, device=DEV)
    out = inpaint.paste_back(packed.to(DEV), pm.to(DEV), shapes[plan.image], plan.windows, fake.to(DEV), k=k, feather=feather, alpha_out=alpha,
                             owner=owner, keys=plan.key)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(alpha.cpu().numpy(), want_alpha) and np.array_equal(want_alpha, _whole_alpha(masks, feather))
    assert not np.array_equal(want[0], packed.numpy())


@pytest.mark.parametrize('k', (1, 2))
@pytest.mark.parametrize('feather', (0, 5))
def test_keyed_membrane_paste_equals_the_unkeyed_chain_once_per_group(k, feather):
    from shgan_amd import inpaint
    images, masks, packed, pm, shapes, plan, fake, groups = _paste_case(k, feather)
    make = dict(info_out=lambda n: torch.full((k, 3), -5, dtype=torch.int32, device=DEV), boxes=lambda n: plan.boxes[n:n + 1])
    want, want_alpha, extras = _per_group(inpaint.paste_back_membrane, k, feather, **make)
    owner = _owner_of(masks, shapes, plan, feather)
    alpha = torch.full((pm.numel(),), 9, dtype=torch.uint8, device=DEV)
    info = torch.full((5 * k, 3), -5, dtype=torch.int32, device=DEV)
    out = inpaint.paste_back_membrane(packed.to(DEV), pm.to(DEV), shapes[plan.image], plan.windows, fake.to(DEV), k=k, feather=feather, alpha_out=alpha,
                                      info_out=info, boxes=plan.boxes, owner=owner, keys=plan.key)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(alpha.cpu().numpy(), want_alpha) and np.array_equal(want_alpha, _whole_alpha(masks, feather))
    assert np.array_equal(info.cpu().numpy(), np.concatenate([e['info_out'].cpu().numpy() for e in extras]))
    assert np.all(info.cpu().numpy()[:, 2] >= 1)


def test_refusals():
    from shgan_amd import _lib, inpaint
    images, masks, packed, pm, shapes, plan, fake, groups = _paste_case(1, 5)
    owner = _owner_of(masks, shapes, plan, 5)
    pk, pmd, fk, n = packed.to(DEV), pm.to(DEV), fake.to(DEV), packed.numel()
    bad_keys = plan.key.copy()
    bad_keys[1] = 0
    big_keys = plan.key.copy()
    big_keys[4] = 256
    for fn in (inpaint.paste_back, inpaint.paste_back_membrane):
        for kw in (dict(owner=owner), dict(keys=plan.key), dict(owner=owner, keys=bad_keys), dict(owner=owner, keys=big_keys),
                   dict(owner=owner[:-1], keys=plan.key), dict(owner=owner.cpu(), keys=plan.key), dict(owner=owner.float(), keys=plan.key),
                   dict(owner=owner, keys=plan.key[:-1])):
            out = torch.full((1, n), 7, dtype=torch.uint8, device=DEV)
            with pytest.raises(_lib.ShgError):
                fn(pk, pmd, shapes[plan.image], plan.windows, fk, feather=5, out=out, **kw)
            assert bool((out == 7).all()), (fn.__name__, sorted(kw))
    lbl = inpaint.label_holes(pmd, shapes, 5)
    for call in (lambda: inpaint.label_holes(pmd.cpu(), shapes, 5), lambda: inpaint.label_holes(pmd, shapes, 33), lambda: inpaint.label_holes(pmd, shapes, 5, 0),
                 lambda: inpaint.label_holes(pmd[:-1], shapes, 5), lambda: inpaint.owner_plane(lbl, pmd, shapes[:1], plan.table),
                 lambda: inpaint.owner_plane(lbl, pmd, shapes, np.array([[0, 0, 256]])), lambda: inpaint.owner_plane(lbl, pmd, shapes, np.array([[2, 0, 1]])),
                 lambda: inpaint.owner_plane(None, pmd, shapes, plan.table), lambda: inpaint.fetch_components(None)):
        with pytest.raises(_lib.ShgError):
            call()


def test_new_sites_do_not_depend_on_fresh_contents_and_stay_inside_their_buffers():
    """('inpaint.py', 'label_holes') -- labels, the scratch plane, the components -- ('inpaint.py', 'owner_plane') -- its scratch plane
    and the result -- and the keyed forms of 'paste_back' / 'paste_back_membrane': the same bits with every fresh allocation pre-filled
    with NaN bytes and with large values, and no guard band touched with every buffer housed between poisoned bands.  The scratch planes
    are the point: they are written at root positions only and read nowhere else."""
    import alloc_fill
    import alloc_guard
    from shgan_amd import inpaint
    sites = {('inpaint.py', 'label_holes'), ('inpaint.py', 'owner_plane'), ('inpaint.py', 'paste_back'), ('inpaint.py', 'paste_back_membrane')}
    images, masks, packed, pm, shapes, plan, fake, groups = _paste_case(2, 5)
    T = _T()
    ragged = hg.pack_case(T, 6)
    rpm, rmoffs = inpaint.pack_masks(ragged)
    rshapes = np.array([(m.shape[0], m.shape[1], 3 * o, o) for m, o in zip(ragged, rmoffs)], np.int64)
    rtable = _keys_of(hg.pack_reference(ragged, 5)[1])

    def run():
        pk, pmd, fk = packed.to(DEV), pm.to(DEV), fake.to(DEV)
        lbl = inpaint.label_holes(pmd, shapes, 5)
        owner = inpaint.owner_plane(lbl, pmd, shapes, plan.table)
        a1, a2 = torch.empty(pm.numel(), dtype=torch.uint8, device=DEV), torch.empty(pm.numel(), dtype=torch.uint8, device=DEV)
        info = torch.empty(10, 3, dtype=torch.int32, device=DEV)
        o1 = inpaint.paste_back(pk, pmd, shapes[plan.image], plan.windows, fk, k=2, feather=5, alpha_out=a1, owner=owner, keys=plan.key)
        o2 = inpaint.paste_back_membrane(pk, pmd, shapes[plan.image], plan.windows, fk, k=2, feather=5, alpha_out=a2, info_out=info, boxes=plan.boxes,
                                         owner=owner, keys=plan.key)
        rp = rpm.to(DEV)
        rl = inpaint.label_holes(rp, rshapes, 5)
        ro = inpaint.owner_plane(rl, rp, rshapes, rtable)
        comps = [torch.from_numpy(inpaint.fetch_components(x)) for x in (lbl, rl)]
        return [lbl.labels, owner, o1, a1, o2, a2, info, rl.labels, ro] + comps
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


def test_inpainter_per_hole_end_to_end(small_g):
    """The reduced-width seeded generator at R = 256, one 481 x 333 photograph with three marks, two of them 10 < 2r = 18 known columns
    apart: two windows; the bytes outside the whole mask's {A > 0} are the original's, the hole bytes are not, and batch = 1 and batch =
    16 give the same bytes."""
    from shgan_amd import inpaint
    rng = np.random.RandomState(17)
    img = ref.random_image(rng, 481, 333)
    mask = ref.mask_with_holes(481, 333, [(40, 70, 30, 60), (50, 62, 70, 90), (400, 430, 250, 300)])
    z = torch.from_numpy(rng.standard_normal((1, 64)).astype(np.float32))
    res = {}
    for batch in (1, 16):
        inp = inpaint.Inpainter(small_g, 256, DEV, feather=8, windows='per_hole', batch=batch)
        res[batch] = inp([img], [mask], z=z)[0]
        assert [(i, k, b) for i, k, _, b in inp.windows_] == [(0, 1, (40, 70, 30, 90)), (0, 2, (400, 430, 250, 300))]
        assert [w for _, _, w, _ in inp.windows_] == [inpaint.window_of_box(b, 481, 333, 256, 0.5, 8) for _, _, _, b in inp.windows_]
    assert np.array_equal(res[1], res[16])
    keep = ref.feather_reference(mask, 8) == 0
    assert np.array_equal(res[1][keep], img[keep]) and not np.array_equal(res[1][mask == 0], img[mask == 0])
    for box in ((40, 70, 30, 60), (50, 62, 70, 90), (400, 430, 250, 300)):
        ya, yb, xa, xb = box
        assert not np.array_equal(res[1][ya:yb, xa:xb], img[ya:yb, xa:xb]), box
