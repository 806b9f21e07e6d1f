"""Places2 input path on the device: (1) the ragged-batch bicubic resize kernel (resize.resize_bicubic_u8) timed with device events after a
warm-up, 16 and 32 images of Places2-like mixed sizes (short side 512, long side 512..1024, both orientations) to 512^2 and 256^2, bytes
moved over time against the 6.3 TB/s copy ceiling; (2) EvalLoop (full-width generator, device masks, stand-in features) on FFHQ-shaped
uint8 batches and on Places2-shaped ragged batches of the same images, alternated in one process, images/s of each.
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
from shgan_amd import configs, datasets, eval_harness as hz, resize as rz  # noqa: E402

DEV = 'cuda:0'
COPY_CEILING_TBS = 6.3


def places2_like(n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        long_side = int(rs.randint(512, 1025))
        h, w = (512, long_side) if i % 2 == 0 else (long_side, 512)
        out.append(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
    return out


def kernel_block(B, R, iters, records):
    imgs = places2_like(B, B * 7 + R)
    packed, shapes = rz.pack_images(imgs)
    dpk = packed.to(DEV)
    flip = np.arange(B) % 2 == 1
    for _ in range(5):
        rz.resize_bicubic_u8(dpk, shapes, R, flip)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = rz.resize_bicubic_u8(dpk, shapes, R, flip)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    ok = all(np.array_equal(out[i].cpu().numpy(), rz.resize_reference(imgs[i], R, flip[i])) for i in range(0, B, max(1, B // 4)))
    nbytes = packed.numel() + B * 3 * R * R
    rec = {'what': 'resize_bicubic_u8 per batch (one launch + its table upload, device events)', 'B': B, 'R': R, 'us_per_batch': round(us, 2),
           'bytes': nbytes, 'TB_per_s': round(nbytes / us * 1e-6, 3), 'of_copy_ceiling': round(nbytes / us * 1e-6 / COPY_CEILING_TBS, 3),
           'sampled_images_exact': bool(ok)}
    records.append(rec)
    print(json.dumps(rec), flush=True)


class RaggedPool:
    """Pre-packed pinned ragged batches (the decode workers' output), cycled like PinnedU8Loader's pool."""

    def __init__(self, ids, b, batches):
        self.ids, self.b, self.batches = list(ids), b, batches

    def __iter__(self):
        for n, b0 in enumerate(range(0, len(self.ids), self.b)):
            src = self.batches[n % len(self.batches)]
            yield datasets.RaggedU8Batch(src.data, src.shapes, src.flip, self.ids[b0:b0 + self.b])


def loop_block(G, R, B, steps, rounds, records):
    pools_imgs = [places2_like(B, 100 + k) for k in range(4)]
    ragged, dense = [], []
    for imgs in pools_imgs:
        packed, shapes = rz.pack_images(imgs)
        ragged.append(datasets.RaggedU8Batch(packed.pin_memory(), shapes, torch.zeros(B, dtype=torch.bool), []))
        dense.append(torch.from_numpy(np.stack([rz.resize_reference(im, R) for im in imgs])).pin_memory())

    class DensePool:
        def __init__(self, ids):
            self.ids = ids

        def __iter__(self):
            for n, b0 in enumerate(range(0, len(self.ids), B)):
                yield dense[n % 4], self.ids[b0:b0 + B]

    def run(kind, n_items):
        loop = hz.EvalLoop(G, DEV, R, n_items, noise_mode='random', seed=0, feature_fn=hz.standin_features, timing=True)
        loader = DensePool(loop.ids) if kind == 'ffhq_shaped_u8' else RaggedPool(loop.ids, B, ragged)
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

    for kind in ('ffhq_shaped_u8', 'places2_ragged'):                # warm-up of both routes
        run(kind, B * 4)
    res = {'ffhq_shaped_u8': [], 'places2_ragged': []}
    for r in range(rounds):
        for kind in (('ffhq_shaped_u8', 'places2_ragged') if r % 2 == 0 else ('places2_ragged', 'ffhq_shaped_u8')):
            res[kind].append(run(kind, B * steps))
    rec = {'what': f'EvalLoop images/s, R={R}, B={B}, {steps} batches per run, {rounds} alternated runs per route (median)', 'R': R, 'B': B}
    for kind, v in res.items():
        rec[kind + '_images_per_s'] = round(float(np.median([a for a, _ in v])), 1)
        rec[kind + '_steady_images_per_s'] = round(float(np.median([s for _, s in v])), 1)
        rec[kind + '_runs'] = [round(a, 1) for a, _ in v]
    rec['places2_over_ffhq'] = round(rec['places2_ragged_images_per_s'] / rec['ffhq_shaped_u8_images_per_s'], 4)
    rec['places2_over_ffhq_steady'] = round(rec['places2_ragged_steady_images_per_s'] / rec['ffhq_shaped_u8_steady_images_per_s'], 4)
    records.append(rec)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=24)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--loop-res', type=int, nargs='*', default=[512])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resize_bench needs a GPU')
    records = []
    for R in (512, 256):
        for B in (16, 32):
            kernel_block(B, R, a.iters, records)
    for R in a.loop_res:
        G = configs.seeded_init_(configs.build_generator(R), seed=0).eval().requires_grad_(False).to(DEV)
        loop_block(G, R, 16, a.steps, a.rounds, records)
        del G
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for r in records:
                fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
