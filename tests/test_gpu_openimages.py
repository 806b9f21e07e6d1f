"""GPU: the OpenImages input path -- the fit-and-pad resize on the device (resize.resize_fit_pad_u8, csrc/resize.hip) against Pillow's
FixResolutionLoader (ds_openimages.py:63-81) byte for byte, the mask rasteriser at 1024 and with content boxes (csrc/mask_raster.hip), and an
``OpenImages`` + ``EvalLoop`` run at R = 1024 against the host route (Pillow on the host, host masks with the box fill, float input)."""
import os

import numpy as np
import numpy.random as npr
import pytest
import torch
from PIL import Image

import shgan_amd  # noqa: F401
from conftest import load_golden
from shgan_amd import data, datasets, masks
from shgan_amd import resize as rz

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _pillow_fit(img, R, flip=False):
    im = Image.fromarray(img)
    w, h = im.size
    if w > R or h > R:
        ratio = R / w if w > h else R / h
        im = im.resize((R, int(h * ratio)) if w > h else (int(w * ratio), R), resample=Image.BICUBIC)
    canvas = np.zeros((R, R, 3), np.uint8)
    canvas[:im.size[1], :im.size[0]] = np.asarray(im)
    out = canvas.transpose(2, 0, 1)
    return np.ascontiguousarray(out[:, :, ::-1] if flip else out)


def _device(images, R, flip=None, stream=None):
    packed, shapes = rz.pack_images(images)
    return rz.resize_fit_pad_u8(packed.to(DEV), shapes, R, flip=flip, stream=stream)


def _short_square(R):
    """The smallest square side above R whose box is one column short (R x (R - 1))."""
    return next(s for s in range(R + 1, 8 * R) if rz.fit_size(s, s, R) == (R, R - 1))


def _cases(rs, R, n):
    """(h, w) at resolution R: pad-only, exactly R, the R - 1 squares, extreme aspect ratios, both orientations, down-scales up to 3x."""
    sq = _short_square(R)
    fixed = [(R, R), (R // 3, R // 2 + 1), (1, 1), (sq, sq), (sq + 1, sq + 1), (R, R // 2), (R // 2, R)]
    fixed += [(3000, 40), (40, 3000)] if R == 1024 else [(3 * R, max(3, R // 25)), (max(3, R // 25), 3 * R)]
    out = list(fixed)
    while len(out) < n:
        long_side = int(rs.randint(R // 2, 3 * R))
        short_side = int(rs.randint(max(1, long_side // 8), long_side + 1))
        out.append((long_side, short_side) if rs.rand() < 0.5 else (short_side, long_side))
    return out


@pytest.mark.parametrize('R,n', [(64, 90), (256, 70), (1024, 40)])
def test_fuzz_is_bit_identical_to_pillow(R, n):
    """Ragged batches of 1..8 images mixing sizes and flips, one launch per batch, each image against Pillow + pad (+ flip)."""
    rs = np.random.RandomState(R)
    cases = _cases(rs, R, n)
    k = done = 0
    while k < len(cases):
        nb = int(rs.randint(1, 9))
        grp = cases[k:k + nb]
        k += nb
        imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in grp]
        flip = rs.rand(len(grp)) < 0.5
        got = _device(imgs, R, flip).cpu().numpy()
        for i, img in enumerate(imgs):
            want = _pillow_fit(img, R, bool(flip[i]))
            assert np.array_equal(got[i], want), (grp[i], bool(flip[i]), int((got[i] != want).sum()))
            done += 1
    assert done == len(cases)


def test_golden_items():
    """The reference's own FixResolutionLoader + formatter canvases (tests/golden/openimages_fit.npz), flips included."""
    g = load_golden('openimages_fit')
    for R in (48, 64):
        idx = [i for i, c in enumerate(g['cases'].tolist()) if c[2] == R]
        got = _device([g[f'in{i}'] for i in idx], R, np.array([bool(g[f'flip{i}']) for i in idx])).cpu().numpy()
        for j, i in enumerate(idx):
            assert np.array_equal(got[j], g[f'x{i}']), i


def test_batch_invariance_and_streams():
    rs = np.random.RandomState(5)
    sizes = [(682, 1024), (1500, 1100), (300, 200), (1024, 1024), (1122, 1122), (40, 3000), (2000, 1333), (900, 1024)]
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    flip = np.array([i % 2 == 1 for i in range(len(imgs))])
    R = 1024
    alone = [_device([im], R, flip[i:i + 1]).cpu().numpy()[0] for i, im in enumerate(imgs)]
    whole = _device(imgs, R, flip).cpu().numpy()
    perm = rs.permutation(len(imgs))
    shuffled = _device([imgs[p] for p in perm], R, flip[perm]).cpu().numpy()
    st = torch.cuda.Stream(DEV)
    with torch.cuda.stream(st):
        side = _device(imgs, R, flip, stream=st)
    torch.cuda.current_stream(DEV).wait_stream(st)
    side = side.cpu().numpy()
    for i in range(len(imgs)):
        assert np.array_equal(whole[i], alone[i]) and np.array_equal(side[i], alone[i])
        assert np.array_equal(shuffled[list(perm).index(i)], alone[i])
        assert np.array_equal(alone[i], _pillow_fit(imgs[i], R, bool(flip[i])))


def test_device_masks_at_1024_are_the_reference_masks():
    """random_masks at s = 1024 == the reference's RandomMask(1024) (golden, 3 seeds) and == the host RandomMask (batch borders crossed)."""
    g = load_golden('openimages_fit')
    for k, seed in enumerate(g['mask_seeds'].tolist()):
        want = np.unpackbits(g[f'rm1024_{k}'])[:1024 * 1024].reshape(1024, 1024)
        np.random.seed(seed)
        got = masks.random_masks(1, 1024, [0.0, 1.0], device=DEV)
        assert np.array_equal(got[0, 0].cpu().numpy().astype(np.uint8), want), seed
    np.random.seed(77)
    got = masks.random_masks(5, 1024, [0.0, 1.0], device=DEV, batch=2).cpu().numpy()
    st = np.random.get_state()[1].copy()
    np.random.seed(77)
    want = np.stack([data.RandomMask(1024, [0.0, 1.0]) for _ in range(5)])
    assert np.array_equal(got, want) and np.array_equal(np.random.get_state()[1], st)
    for s in (544, 992):                                    # other multiples of 32 above 512
        np.random.seed(s)
        got = masks.random_masks(2, s, [0.0, 1.0], device=DEV).cpu().numpy()
        np.random.seed(s)
        assert np.array_equal(got, np.stack([data.RandomMask(s, [0.0, 1.0]) for _ in range(2)])), s


def test_boxed_masks_are_the_numpy_fill_with_counts_before_it():
    boxes = np.array([(1024, 1023), (682, 1024), (1024, 13), (500, 700), (1, 1), (1024, 1024)], np.int32)
    for s, bx in ((1024, boxes), (256, np.minimum(boxes, 256)), (64, np.minimum(boxes, 64))):
        np.random.seed(s)
        recs, offs, flips = [], [0], []
        for _ in range(len(bx)):
            r, f0, f1 = masks.mask_attempt_records(s, [0.0, 1.0])
            recs.append(r)
            offs.append(offs[-1] + len(r))
            flips.append((int(f0), int(f1)))
        rec = np.concatenate(recs)
        plain, h0 = masks.rasterize(rec, offs, flips, s, DEV)
        boxed, h1 = masks.rasterize(rec, offs, flips, s, DEV, boxes=bx)
        want = plain.cpu().numpy()
        for k, box in enumerate(bx):
            datasets.fill_outside_box(want[k, 0], box)
        assert np.array_equal(boxed.cpu().numpy(), want), s
        assert torch.equal(h0.cpu(), h1.cpu()) and int(h0.sum()) > 0
        assert torch.equal(h0.cpu(), (1 - plain).sum(dim=(1, 2, 3)).to(torch.int32).cpu())
    # random_masks with boxes: the same RNG stream and the same masks as without, then filled
    np.random.seed(3)
    a = masks.random_masks(6, 1024, [0.0, 1.0], device=DEV, batch=4).cpu().numpy()
    np.random.seed(3)
    b = masks.random_masks(6, 1024, [0.0, 1.0], device=DEV, batch=4, boxes=boxes).cpu().numpy()
    for k, box in enumerate(boxes):
        datasets.fill_outside_box(a[k, 0], box)
    assert np.array_equal(a, b)


def _tree(root, rs):
    """A validation tree of Pillow-written JPEG / PNG files of mixed sizes: larger than 1024 both ways, smaller, exact, an R - 1 square."""
    sizes = [(1500, 1100), (700, 900), (1122, 1122), (1024, 768), (2000, 1333), (400, 1700), (1024, 1024)]
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 7) % 256], -1).astype(np.uint8)
        img = np.clip(img.astype(np.int32) + rs.randint(-20, 21, size=img.shape), 0, 255).astype(np.uint8)
        d = os.path.join(root, 'validation', 'sub' if i % 2 else '')
        os.makedirs(d, exist_ok=True)
        Image.fromarray(img).save(os.path.join(d, f'im{i:02d}.' + ('jpg' if i % 3 else 'png')), **({'quality': 90} if i % 3 else {}))


def test_openimages_eval_loop_at_1024_equals_the_host_route(tmp_path):
    """OpenImages + DeviceFeeder (device fit-and-pad, device masks with the box fill) in EvalLoop at R = 1024 == Pillow's
    FixResolutionLoader on the host + host RandomMask with the box fill + float input, same seed and per-id latents: the same generator
    input x4, uint8 composites, PSNR and SSIM."""
    from shgan_amd import configs, eval_harness as hz
    _tree(str(tmp_path), np.random.RandomState(3))
    R, b = 1024, 3
    G = configs.seeded_init_(configs.build_generator(R, ch_base=4096, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5,
                             noise_strength=0.1, bias_std=0.1).eval().requires_grad_(False).to(DEV)
    ds = datasets.openimages_val_1024(str(tmp_path))
    n = len(ds)
    assert n == 7

    def latents(ids, bb):
        out = torch.empty(bb, 64)
        gen = torch.Generator()
        for k, i in enumerate(ids):
            gen.manual_seed(900 + sum(map(ord, str(i))))
            out[k].normal_(generator=gen)
        return out.to(DEV)

    def run(loader, device_masks):
        x4s = []

        def step(x4, z, out):
            x4s.append(x4.clone())
            return hz.run_generator(G, x4, z, noise_mode='const', out=out)
        loop = hz.EvalLoop(G, DEV, R, n, noise_mode='const', latent_fn=latents, step_fn=step, metrics=('psnr', 'ssim'),
                           device_masks=device_masks)
        npr.seed(21)
        loop.run(loader)
        images, _ = loop.gather()
        torch.cuda.synchronize()
        return torch.cat(x4s).cpu(), images.cpu(), loop.image_metrics

    dev = run(torch.utils.data.DataLoader(ds, batch_size=b, shuffle=False, num_workers=0, collate_fn=datasets.collate_ragged), True)

    def host_loader():
        for k in range(0, n, b):
            items = [ds.load_info[i] for i in range(k, min(k + b, n))]
            xs, ms = [], []
            for e in items:
                im = Image.open(e['image_path']).convert('RGB')
                xs.append(torch.from_numpy(_pillow_fit(np.asarray(im), R)).to(torch.float32).div(255) * 2 - 1)
            for e, x in zip(items, xs):                      # the reference's formatter: RandomMask, then the box fill
                w, h = Image.open(e['image_path']).size
                m = data.RandomMask(R, [0.0, 1.0])[0]
                bh, bw = rz.fit_size(h, w, R)
                m[:, bw:] = 1.0
                m[bh:, :] = 1.0
                ms.append(torch.from_numpy(m))
            yield torch.stack(xs), torch.stack(ms), [e['unique_id'] for e in items]
    host = run(host_loader(), False)
    assert any(rz.fit_size(*Image.open(e['image_path']).size[::-1], R) != (R, R) for e in ds.load_info)
    assert torch.equal(dev[0], host[0]), 'generator input x4 differs'
    assert torch.equal(dev[1], host[1]), int((dev[1] != host[1]).sum())
    for m in ('psnr', 'ssim'):
        a, c = torch.as_tensor(dev[2][m + '_per_image']).cpu(), torch.as_tensor(host[2][m + '_per_image']).cpu()
        assert a.numel() == n and torch.equal(a, c) and float(dev[2][m]) == float(host[2][m]), m


def test_feeder_host_masks_and_flips(tmp_path):
    """The train variant (random flips) with the dataset's host masks at R = 64: DeviceFeeder's real images are Pillow + pad + the item's
    flip of the whole canvas, its masks the items' masks (box fill with the unflipped box)."""
    rs = np.random.RandomState(4)
    d = tmp_path / 'train'
    d.mkdir()
    for i, (h, w) in enumerate([(90, 120), (98, 98), (40, 50), (64, 200), (300, 70)]):
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(str(d / f'c{i}.png'))
    ds = datasets.OpenImages(str(tmp_path), 'train', resolution=64, random_flip=True, host_masks=True)
    npr.seed(8)
    items = [ds[i] for i in range(len(ds))]
    npr.seed(8)
    feeder = datasets.DeviceFeeder(DEV, 64)
    seen = 0
    for x4, real, mask, ids in feeder(torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0, collate_fn=datasets.collate_ragged)):
        torch.cuda.synchronize()
        for k, uid in enumerate(ids):
            it = items[seen + k]
            assert uid == it['unique_id']
            assert np.array_equal(real[k].cpu().numpy(), _pillow_fit(it['image'], 64, it['flip']))
            assert np.array_equal(mask[k, 0].cpu().numpy(), it['mask'])
        seen += len(ids)
    assert seen == 5 and any(it['flip'] for it in items) and not all(it['flip'] for it in items)
