"""GPU: the Places2 input path -- ragged-batch bicubic resize on the device (resize.resize_bicubic_u8, csrc/resize.hip) against Pillow's
``Image.resize([R, R], BICUBIC)`` (FixResolutionLoader, ds_places2.py:90-103) byte for byte, and a ``Places2`` + ``EvalLoop`` run against
the host route (Pillow on the host, float input)."""
import os

import numpy as np
import numpy.random as npr
import pytest
import torch

import shgan_amd  # noqa: F401
from conftest import load_golden
from shgan_amd import resize as rz

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _pillow(img, R, flip=False):
    from PIL import Image
    out = np.asarray(Image.fromarray(img).resize([R, R], Image.BICUBIC)).transpose(2, 0, 1)
    return np.ascontiguousarray(out[:, :, ::-1] if flip else out)


def _device(images, R, flip=None, stream=None):
    packed, shapes = rz.pack_images(images)
    return rz.resize_bicubic_u8(packed.to(DEV), shapes, R, flip=flip, stream=stream)


def _cases(rs, n):
    """(h, w, R): down-scale 1..6 and up-sampling, equal sizes, one axis only, odd sizes."""
    out = []
    for i in range(n):
        R = int(rs.choice([256, 512, 37, 100]))
        f = [rs.uniform(0.2, 1.0), rs.uniform(1.0, 2.0), rs.uniform(2.0, 6.0)][i % 3]
        h, w = max(1, int(R * f * rs.uniform(0.8, 1.25))), max(1, int(R * f * rs.uniform(0.8, 1.25)))
        if i % 7 == 3:
            h = R
        if i % 11 == 5:
            w = R
        if i % 13 == 6:
            h = w = R
        if h * w > 1200 * 1200:                                # keep the host side of the test quick
            h, w = min(h, 1200), min(w, 1200)
        out.append((h, w, R))
    return out


def test_fuzz_is_bit_identical_to_pillow():
    """>= 200 seeded cases in ragged batches of 1..8 images that mix sizes and flips (one launch per batch and R)."""
    rs = np.random.RandomState(11)
    cases = _cases(rs, 216)
    done, k = 0, 0
    while k < len(cases):
        nb = int(rs.randint(1, 9))
        grp = cases[k:k + nb]
        k += nb
        for R in sorted({c[2] for c in grp}):
            sub = [c for c in grp if c[2] == R]
            imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w, _ in sub]
            flip = rs.rand(len(sub)) < 0.5
            got = _device(imgs, R, flip).cpu().numpy()
            for i, img in enumerate(imgs):
                want = _pillow(img, R, bool(flip[i]))
                assert np.array_equal(got[i], want), (sub[i], bool(flip[i]), int((got[i] != want).sum()))
                done += 1
    assert done >= 200


def test_golden_fixture():
    g = load_golden('places2_resize')
    cases = g['cases']
    for R in sorted(set(int(c[2]) for c in cases)):
        idx = [i for i, c in enumerate(cases) if int(c[2]) == R]
        got = _device([g[f'in{i}'] for i in idx], R).cpu().numpy()
        for j, i in enumerate(idx):
            assert np.array_equal(got[j], g[f'out{i}']), tuple(cases[i])
    # one image per launch as well
    for i, c in enumerate(cases):
        assert np.array_equal(_device([g[f'in{i}']], int(c[2])).cpu().numpy()[0], g[f'out{i}'])


def test_batch_invariance_and_streams():
    """An image's bytes do not depend on its neighbours or its place in the batch; a non-default stream gives the same bytes."""
    rs = np.random.RandomState(5)
    sizes = [(512, 683), (768, 512), (300, 200), (512, 512), (777, 1311), (90, 64), (512, 700)]
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]
    flip = np.array([i % 2 == 1 for i in range(len(imgs))])
    for R in (256, 512):
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
            assert np.array_equal(alone[i], _pillow(imgs[i], R, bool(flip[i])))


def _jpeg_tree(root, rs):
    from PIL import Image
    d = os.path.join(root, 'val_large', 'a', 'b')
    os.makedirs(d)
    sizes = [(300, 420), (256, 256), (512, 341), (200, 180), (640, 480), (256, 300), (333, 257)]
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 7) % 256], -1).astype(np.uint8)
        img = np.clip(img.astype(np.int32) + rs.randint(-20, 21, size=img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(d if i % 2 else os.path.join(root, 'val_large'), f'im{i:02d}.jpg'), quality=90)


def test_places2_eval_loop_equals_the_host_route(tmp_path):
    """Places2 + DeviceFeeder (device resize, device masks) in EvalLoop == Pillow's resize on the host + float input, same seed and latents:
    the same generator input x4, uint8 composites, PSNR and SSIM."""
    from PIL import Image
    from shgan_amd import configs, datasets, eval_harness as hz
    _jpeg_tree(str(tmp_path), np.random.RandomState(3))
    R, b = 256, 3
    G = configs.seeded_init_(configs.build_generator(R, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1).eval().requires_grad_(False).to(DEV)
    ds = datasets.places2_val256_inpainting(str(tmp_path))
    n = len(ds)
    assert n == 7

    def latents(ids, bb):
        out = torch.empty(bb, 64)
        g = torch.Generator()
        for k, i in enumerate(ids):
            g.manual_seed(900 + sum(map(ord, str(i))))
            out[k].normal_(generator=g)
        return out.to(DEV)

    def run(loader):
        x4s = []

        def step(x4, z, out):
            x4s.append(x4.clone())
            return hz.run_generator(G, x4, z, noise_mode='const', out=out)
        loop = hz.EvalLoop(G, DEV, R, n, noise_mode='const', latent_fn=latents, step_fn=step, metrics=('psnr', 'ssim'))
        npr.seed(21)
        loop.run(loader)
        images, _ = loop.gather()
        torch.cuda.synchronize()
        return torch.cat(x4s).cpu(), images.cpu(), loop.image_metrics

    dev = run(torch.utils.data.DataLoader(ds, batch_size=b, shuffle=False, num_workers=0, collate_fn=datasets.collate_ragged))

    def host_loader():
        for k in range(0, n, b):
            items = [ds.load_info[i] for i in range(k, min(k + b, n))]
            xs = []
            for e in items:
                im = Image.open(e['image_path']).convert('RGB').resize([R, R], Image.BICUBIC)
                xs.append(torch.from_numpy(np.asarray(im).transpose(2, 0, 1).copy()).to(torch.float32).div(255) * 2 - 1)
            yield torch.stack(xs), [e['unique_id'] for e in items]
    host = run(host_loader())
    assert torch.equal(dev[0], host[0]), 'generator input x4 differs'
    assert torch.equal(dev[1], host[1]), int((dev[1] != host[1]).sum())
    for m in ('psnr', 'ssim'):
        a, c = torch.as_tensor(dev[2][m + '_per_image']).cpu(), torch.as_tensor(host[2][m + '_per_image']).cpu()
        assert a.numel() == n and torch.equal(a, c) and float(dev[2][m]) == float(host[2][m]), m


def test_feeder_host_masks_and_flips(tmp_path):
    """The challenge variant (random flips) with the formatter's host masks: DeviceFeeder's real images are Pillow's resize + the item's
    flip, its masks the items' masks."""
    from PIL import Image
    from shgan_amd import datasets
    rs = np.random.RandomState(4)
    d = tmp_path / 'data_challenge'
    d.mkdir()
    for i, (h, w) in enumerate([(300, 420), (256, 256), (512, 341), (90, 120), (256, 700)]):
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(str(d / f'c{i}.png'))
    ds = datasets.places2_challenge256_inpainting(str(tmp_path), host_masks=True)
    npr.seed(8)
    items = [ds[i] for i in range(len(ds))]
    npr.seed(8)
    feeder = datasets.DeviceFeeder(DEV, 256)
    seen = 0
    for x4, real, mask, ids in feeder(torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0, collate_fn=datasets.collate_ragged)):
        torch.cuda.synchronize()
        for k, uid in enumerate(ids):
            it = items[seen + k]
            assert uid == it['unique_id']
            assert np.array_equal(real[k].cpu().numpy(), _pillow(it['image'], 256, it['flip']))
            assert np.array_equal(mask[k, 0].cpu().numpy(), it['mask'])
        seen += len(ids)
    assert seen == 5 and any(it['flip'] for it in items) and not all(it['flip'] for it in items)
