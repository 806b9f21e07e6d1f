"""OpenImages input path on the device at R = 1024: (1) the fit-and-pad resize kernel (resize.resize_fit_pad_u8) timed with device events
after a warm-up, batches of 8 OpenImages-like images (long side 1024..3000, both orientations, every fourth one smaller than R), bytes moved
over time against the 6.3 TB/s copy ceiling; (2) device masks/s at 1024 (masks.random_masks, with content boxes) against the host
``RandomMask``; (3) EvalLoop (full-width shgan_g1024, device masks, stand-in features) on OpenImages-shaped ragged batches and on uint8
tensor batches of the same images padded on the host, alternated in one process, images/s of each and their ratio.
Prints one JSON line per measurement; ``--out`` also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shgan_amd  # noqa: E402,F401
from shgan_amd import configs, data, datasets, eval_harness as hz, masks, resize as rz  # noqa: E402

DEV = 'cuda:0'
COPY_CEILING_TBS = 6.3
R = 1024


def openimages_like(n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        if i % 4 == 3:
            h, w = int(rs.randint(300, 1025)), int(rs.randint(300, 1025))
        else:
            long_side = int(rs.randint(1024, 3001))
            short_side = int(long_side * rs.uniform(0.5, 0.85))
            h, w = (short_side, long_side) if i % 2 == 0 else (long_side, short_side)
        out.append(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
    return out


def kernel_block(B, iters, records):
    imgs = openimages_like(B, B * 7 + R)
    packed, shapes = rz.pack_images(imgs)
    dpk = packed.to(DEV)
    flip = np.arange(B) % 2 == 1
    for _ in range(5):
        rz.resize_fit_pad_u8(dpk, shapes, R, flip)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = rz.resize_fit_pad_u8(dpk, shapes, R, flip)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    ok = all(np.array_equal(out[i].cpu().numpy(), rz.fit_reference(imgs[i], R, flip[i])) for i in range(0, B, max(1, B // 4)))
    nbytes = packed.numel() + B * 3 * R * R
    rec = {'what': 'resize_fit_pad_u8 per batch (one launch + its table upload, device events)', 'B': B, 'R': R,
           'sizes': [list(im.shape[:2]) for im in imgs], 'us_per_batch': round(us, 2), 'bytes': nbytes,
           'TB_per_s': round(nbytes / us * 1e-6, 3), 'of_copy_ceiling': round(nbytes / us * 1e-6 / COPY_CEILING_TBS, 3),
           'sampled_images_exact': bool(ok)}
    records.append(rec)
    print(json.dumps(rec), flush=True)


def mask_block(n_dev, n_host, records):
    boxes = np.array([rz.fit_size(im.shape[0], im.shape[1], R) for im in openimages_like(n_dev, 5)], np.int32)
    np.random.seed(1)
    masks.random_masks(16, R, [0.0, 1.0], device=DEV, boxes=boxes[:16])
    torch.cuda.synchronize()
    np.random.seed(2)
    t0 = time.perf_counter()
    masks.random_masks(n_dev, R, [0.0, 1.0], device=DEV, boxes=boxes)
    torch.cuda.synchronize()
    dev_s = time.perf_counter() - t0
    np.random.seed(2)
    t0 = time.perf_counter()
    for _ in range(n_host):
        data.RandomMask(R, [0.0, 1.0])
    host_s = time.perf_counter() - t0
    rec = {'what': 'masks/s at 1024: masks.random_masks (host draws + HIP rasteriser, content boxes) vs host RandomMask (one thread)',
           'device_masks_per_s': round(n_dev / dev_s, 1), 'host_masks_per_s': round(n_host / host_s, 2),
           'device_over_host': round((n_dev / dev_s) / (n_host / host_s), 1), 'n_device': n_dev, 'n_host': n_host}
    records.append(rec)
    print(json.dumps(rec), flush=True)


class RaggedPool:
    """Pre-packed pinned ragged batches (the decode workers' output), cycled."""

    def __init__(self, ids, b, batches):
        self.ids, self.b, self.batches = list(ids), b, batches

    def __iter__(self):
        for n, b0 in enumerate(range(0, len(self.ids), self.b)):
            src = self.batches[n % len(self.batches)]
            yield datasets.RaggedU8Batch(src.data, src.shapes, src.flip, self.ids[b0:b0 + self.b], fit=True, content_size=src.content_size)


def loop_block(G, B, steps, rounds, records):
    pools_imgs = [openimages_like(B, 100 + k) for k in range(4)]
    ragged, dense = [], []
    for imgs in pools_imgs:
        packed, shapes = rz.pack_images(imgs)
        cs = torch.tensor([rz.fit_size(im.shape[0], im.shape[1], R) for im in imgs], dtype=torch.int32)
        ragged.append(datasets.RaggedU8Batch(packed.pin_memory(), shapes, torch.zeros(B, dtype=torch.bool), [], fit=True, content_size=cs))
        dense.append(torch.from_numpy(np.stack([rz.fit_reference(im, R) for im in imgs])).pin_memory())

    class DensePool:
        def __init__(self, ids):
            self.ids = ids

        def __iter__(self):
            for n, b0 in enumerate(range(0, len(self.ids), B)):
                yield dense[n % 4], self.ids[b0:b0 + B]

    def run(kind, n_items):
        loop = hz.EvalLoop(G, DEV, R, n_items, noise_mode='random', seed=0, feature_fn=hz.standin_features, timing=True)
        loader = DensePool(loop.ids) if kind == 'tensor_u8' else RaggedPool(loop.ids, B, ragged)
        np.random.seed(2000)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(loader)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        evs = loop.batch_done_events
        k0, k1 = len(evs) // 4, len(evs) - 1 - len(evs) // 4
        steady = evs[k0].elapsed_time(evs[k1]) / (k1 - k0)
        return n_items / dt, B / steady * 1e3

    for kind in ('tensor_u8', 'openimages_ragged'):                    # warm-up of both routes
        run(kind, B * 4)
    res = {'tensor_u8': [], 'openimages_ragged': []}
    for r in range(rounds):
        for kind in (('tensor_u8', 'openimages_ragged') if r % 2 == 0 else ('openimages_ragged', 'tensor_u8')):
            res[kind].append(run(kind, B * steps))
    rec = {'what': f'EvalLoop images/s, R={R}, B={B}, {steps} batches per run, {rounds} alternated runs per route (median)', 'R': R, 'B': B}
    for kind, v in res.items():
        rec[kind + '_images_per_s'] = round(float(np.median([a for a, _ in v])), 2)
        rec[kind + '_steady_images_per_s'] = round(float(np.median([s for _, s in v])), 2)
        rec[kind + '_runs'] = [round(a, 2) for a, _ in v]
    rec['openimages_over_tensor'] = round(rec['openimages_ragged_images_per_s'] / rec['tensor_u8_images_per_s'], 4)
    rec['openimages_over_tensor_steady'] = round(rec['openimages_ragged_steady_images_per_s'] / rec['tensor_u8_steady_images_per_s'], 4)
    records.append(rec)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--no-loop', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('openimages_bench needs a GPU')
    records = []
    kernel_block(8, a.iters, records)
    mask_block(64, 8, records)
    if not a.no_loop:
        G = configs.seeded_init_(configs.build_generator(R), seed=0).eval().requires_grad_(False).to(DEV)
        loop_block(G, a.batch, a.steps, a.rounds, records)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for r in records:
                fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
