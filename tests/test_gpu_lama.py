"""GPU: the LaMa thin / medium / thick masks on the device (csrc/mask_lama.hip, ``masks.lama_masks``) against the restatement of
OpenCV's thick line (tests/lama_cv_ref.py) and against the host path (``data.LamaMask``), bit for bit, hole counts included; the
plumbing through ``DeviceFeeder`` and ``EvalLoop``.  Every refused argument is refused on the host, before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import lama_cv_ref as cv

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
S = 64                      # the smallest canvas with two words per row of the bit plane

# (x0, y0, x1, y1, t) at s = 64
LINES = [
    (5, 20, 50, 20, 7), (30, 5, 30, 55, 8), (5, 5, 50, 50, 9), (5, 50, 50, 5, 10),                   # horizontal, vertical, +-45 degrees
    (3, 10, 60, 25, 5), (10, 3, 25, 60, 6), (60, 25, 3, 10, 5), (25, 60, 10, 3, 6),                 # x-major, y-major, both directions
    (8, 40, 55, 12, 40), (20, 30, 44, 34, 33), (12, 12, 14, 50, 21), (50, 8, 20, 44, 16), (31, 33, 33, 31, 28),      # t odd and even, 5 .. 40
    (10, 10, 50, 50, 254),                                                                           # covers the whole canvas
    (20, 20, 20, 20, 11), (0, 0, 0, 0, 6), (64, 64, 64, 64, 9),                                      # zero length
    (40, 10, 64, 30, 12), (10, 40, 30, 64, 13), (64, 0, 64, 64, 5), (0, 64, 64, 64, 6),              # end points at x == 64, y == 64
    (2, 30, 2, 40, 20), (62, 30, 62, 40, 20), (30, 2, 40, 2, 20), (30, 62, 40, 62, 20),              # quads leaving through each side
    (2, 2, 6, 6, 30), (62, 2, 58, 6, 30), (2, 62, 6, 58, 30), (62, 62, 58, 58, 30),                  # ... and each corner
    (0, 10, 10, 0, 25), (64, 50, 50, 64, 25), (54, 0, 64, 12, 23), (0, 52, 14, 64, 22),
    (-10, 30, 80, 35, 9), (30, -10, 35, 80, 9), (-30, -10, 90, 70, 15), (90, -12, -20, 75, 14),      # through the canvas: clipLine's second pass
    (66, 30, 100, 30, 10), (30, -3, 30, -40, 12),                                                    # a quad wholly off canvas beside its on-canvas circle
]
RECTS = [(10, 30, 20, 50), (50, 70, -5, 10), (0, 64, 63, 64), (31, 33, 0, 64)]                       # (x0, x1, y0, y1)


def line_rec(c):
    return [1, *c, 0, 0]


def rect_rec(r):
    return [0, *r, 0, 0, 0]


def ref_painted(recs, s):
    img = np.zeros((s, s), np.uint8)
    for r in recs:
        if r[0] == 0:
            img[max(r[3], 0):max(r[4], 0), max(r[1], 0):max(r[2], 0)] = 1
        else:
            img |= cv.draw([r[1:6]], s)
    return img


def device_painted(per_mask, s):
    from shgan_amd import masks
    offs = np.cumsum([0] + [len(m) for m in per_mask])
    recs = np.asarray([r for m in per_mask for r in m], dtype=np.int32).reshape(-1, 8)
    mask, holes = masks.lama_rasterize(recs, offs, s, DEV)
    m = mask.cpu().numpy()
    assert m.dtype == np.float32 and m.shape == (len(per_mask), 1, s, s) and set(np.unique(m)) <= {0.0, 1.0}
    return (1 - m[:, 0]).astype(np.uint8), holes.cpu().numpy()


def test_hand_made_records_equal_the_restatement():
    import shgan_amd  # noqa: F401
    per_mask = [[line_rec(c)] for c in LINES] + [[rect_rec(r)] for r in RECTS] + [[]]
    per_mask.append([line_rec(c) for c in LINES[:13]] + [rect_rec(RECTS[0])])          # many records in one mask: every wave has work
    per_mask.append([line_rec(c) for c in LINES[14:]] + [rect_rec(r) for r in RECTS[1:]])
    cv.TRACE = set()
    try:
        want = [ref_painted(m, S) for m in per_mask]
        branches = set(cv.TRACE)
    finally:
        cv.TRACE = None
    assert branches == {'inside', 'same side', 'clipped', 'rejected after clipping', 'p1 top', 'p1 bottom', 'p2 top', 'p2 bottom', 'p1 left',
                        'p1 right', 'p2 left', 'p2 right'}, branches                     # every branch of clipLine runs
    got, holes = device_painted(per_mask, S)
    for k, m in enumerate(per_mask):
        assert np.array_equal(got[k], want[k]), (k, m[:1], int((got[k] != want[k]).sum()))
        assert int(holes[k]) == int(want[k].sum()), (k, m[:1])
    k_none, k_full = len(LINES) + len(RECTS), LINES.index((10, 10, 50, 50, 254))
    assert not got[k_none].any() and holes[k_none] == 0                                  # no records: all keep, zero holes
    assert got[k_full].all() and holes[k_full] == S * S                                  # t = 254: all hole


@pytest.mark.parametrize('kind,res', [(k, r) for r in (256, 512) for k in ('thin', 'medium', 'thick')])
def test_generator_equals_the_host_path(kind, res):
    import shgan_amd  # noqa: F401
    from shgan_amd import data, masks
    seed = {'thin': 4, 'medium': 1, 'thick': 2}[kind] + res
    np.random.seed(seed)
    mask, holes = masks.lama_masks(4, res, kind, device=DEV)
    witness = int(np.random.randint(2 ** 31))
    np.random.seed(seed)
    want = np.stack([data.LamaMask(res, kind) for _ in range(4)])
    assert int(np.random.randint(2 ** 31)) == witness
    assert mask.dtype == torch.float32 and tuple(mask.shape) == (4, 1, res, res) and holes.dtype == torch.int32
    got = mask.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(holes.cpu().numpy(), (want == 0).sum(axis=(1, 2, 3)))
    mask2, _ = masks.lama_masks(1, res, 'lama_' + kind, device=DEV)                     # the mask_kind spelling
    assert tuple(mask2.shape) == (1, 1, res, res)


def test_a_mask_does_not_depend_on_its_batch():
    import shgan_amd  # noqa: F401
    from shgan_amd import masks
    np.random.seed(31)
    per_mask = [masks.lama_mask_records(256, masks.LAMA_SETTINGS[(k, 256)]).tolist() for k in ('thin', 'thick', 'medium', 'thin', 'medium')]
    got, holes = device_painted(per_mask, 256)
    for k, m in enumerate(per_mask):
        alone, h1 = device_painted([m], 256)
        assert np.array_equal(alone[0], got[k]) and int(h1[0]) == int(holes[k]) == int(got[k].sum()), k


def test_side_stream_and_holes_not_zeroed():
    import shgan_amd  # noqa: F401
    from shgan_amd import _lib, masks
    per_mask = [[line_rec(LINES[8])], [], [rect_rec(RECTS[0]), line_rec(LINES[2])]]
    want = [ref_painted(m, S) for m in per_mask]
    st = torch.cuda.Stream(DEV)
    with torch.cuda.stream(st):
        got, holes = device_painted(per_mask, S)                                         # the launch goes to the current stream
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and [int(h) for h in holes] == [int(w.sum()) for w in want]
    # the entry point itself, with garbage in ``holes`` and in ``mask``
    rec = masks.lama_quad_offsets(np.asarray([r for m in per_mask for r in m], np.int32))
    off = np.array([0, 1, 1, 3], np.int32)
    rec_d, off_d = torch.from_numpy(rec.reshape(-1)).to(DEV), torch.from_numpy(off).to(DEV)
    tab_d = torch.from_numpy(masks.lama_circle_table().reshape(-1).copy()).to(DEV)
    mask = torch.full((3, 1, S, S), 7.0, device=DEV)
    holes = torch.full((3,), 123456, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                          # noqa: E731
    with torch.cuda.stream(st):
        rc = _lib.get_lib().shg_mask_lama_f32(rec.ctypes.data, off.ctypes.data, p(rec_d), p(off_d), p(tab_d), 512, p(mask), p(holes), 3, 3, S,
                                              ctypes.c_void_p(st.cuda_stream))
    st.synchronize()
    assert rc == 0
    assert [int(h) for h in holes.cpu()] == [int(w.sum()) for w in want]
    assert np.array_equal(1 - mask.cpu().numpy()[:, 0], np.stack(want).astype(np.float32))


def test_refusals_come_before_any_launch():
    import shgan_amd  # noqa: F401
    from shgan_amd import _lib, datasets, masks
    ok = np.asarray([line_rec(LINES[0])], np.int32)
    for s in (48, 1024):
        with pytest.raises(_lib.ShgError):
            masks.lama_rasterize(ok, [0, 1], s, DEV)
    with pytest.raises(_lib.ShgError):
        masks.lama_rasterize(np.asarray([line_rec((5, 5, 20, 20, 1))], np.int32), [0, 1], S, DEV)
    with pytest.raises(_lib.ShgError):
        masks.lama_masks(2, 1024, 'thin', device=DEV)
    # a batch with content boxes (OpenImages) and a LaMa kind: refused while staging, before the resize
    items = [{'image': np.zeros((40, 50, 3), np.uint8), 'flip': False, 'unique_id': str(k), 'content_size': (40, 50)} for k in range(2)]
    feeder = datasets.DeviceFeeder(DEV, 256, device_masks=True, mask_kind='lama_thick')
    with pytest.raises(_lib.ShgError):
        list(feeder([datasets.collate_ragged(items)]))
    torch.cuda.synchronize()


def test_device_feeder_draws_the_formatters_masks():
    import shgan_amd  # noqa: F401
    from shgan_amd import datasets
    rs = np.random.RandomState(4)
    batches = [(torch.from_numpy(rs.rand(n, 3, 256, 256).astype(np.float32) * 2 - 1), [f'i{n}_{k}' for k in range(n)]) for n in (3, 2)]
    np.random.seed(12)
    out = list(datasets.DeviceFeeder(DEV, 256, device_masks=True, mask_kind='lama_thin', hole_range=(0.4, 0.5))(batches))   # hole_range: ignored
    after = int(np.random.randint(2 ** 31))
    np.random.seed(12)
    fmt = datasets.LamaMaskFormatter(random_flip=False, resolution=256, type='thin')
    for (x4, xd, md, ids), (x, want_ids) in zip(out, batches):
        want = torch.from_numpy(np.stack([fmt({'image': (x[k] + 1) / 2, 'unique_id': want_ids[k]})[1] for k in range(len(want_ids))]))
        assert ids == want_ids and torch.equal(md.cpu()[:, 0], want)
        assert torch.equal(x4.cpu(), torch.cat([want[:, None] - 0.5, x * want[:, None]], dim=1))
    assert int(np.random.randint(2 ** 31)) == after


@pytest.fixture(scope='module')
def small_g():
    import shgan_amd  # noqa: F401
    from shgan_amd import configs
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1)
    return G.eval().requires_grad_(False).to(DEV)


def _latents(ids, b, z_dim=64):
    out = torch.empty(b, z_dim)
    g = torch.Generator()
    for k, i in enumerate(ids):
        g.manual_seed(500 + int(i))
        out[k].normal_(generator=g)
    return out.to(DEV)


def test_eval_loop_with_lama_masks(small_g):
    """Two batches end to end: the loop's result buffer == the plain per-batch calls with ``masks.lama_masks`` from the same RNG state."""
    from shgan_amd import eval_harness as hz, masks
    n_items, b, R = 7, 4, 256
    loop = hz.EvalLoop(small_g, DEV, R, n_items, noise_mode='const', latent_fn=_latents, mask_kind='lama_medium')
    np.random.seed(21)
    loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=9))
    images, _ = loop.gather()
    torch.cuda.synchronize()
    np.random.seed(21)
    outs = []
    for img, ids in hz.PinnedU8Loader(list(range(n_items)), b, R, seed=9):
        m, _ = masks.lama_masks(len(ids), R, 'medium', device=DEV)
        x = hz.assemble_input((img.to(torch.float32).div(255) * 2 - 1).to(DEV), m)
        outs.append(hz.run_generator(small_g, x, _latents(ids, len(ids)), noise_mode='const'))
    want = torch.cat(outs)
    assert images.dtype == torch.uint8 and tuple(images.shape) == (n_items, 3, R, R) and loop.seen == n_items
    assert torch.equal(images, want), int((images != want).sum())
