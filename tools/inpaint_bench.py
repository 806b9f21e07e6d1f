"""``inpaint.gather_windows`` and ``inpaint.paste_back`` (csrc/inpaint.hip) timed with device events after a warm-up, against the same
steps composed from torch operators on the same device.  Workload: 8 photographs of 3000 x 2000 with a hole box of about 900 x 700 each
(window 1800 x 1800 by ``plan_window``), R = 512, feather = 16, K = 1 and K = 4.

Per step three timings: the kernel alone (the C entry point in a loop on a table already on the device: back-to-back launches), the
Python call as ``Inpainter`` pays it (table pinned and uploaded per call; ``paste_back`` also makes its K copies of the originals), and
the torch composition:
  gather   per image: crop, ``F.interpolate(bicubic, antialias=True)`` down to R, round + clamp + cast; the mask by ``adaptive_max_pool2d``
           of the hole;
  paste    per image and sample: ``F.interpolate(bicubic)`` up to the window, the ramp as feather + 1 running 3 x 3 max-pools of the hole,
           scale, blend, truncating cast, the window written into a clone of the original.
(The torch steps are the closest operators, not the same arithmetic: torch's bicubic uses a = -0.75 and floating point.)

Bytes a kernel must move, over its time, beside the 6.0 / 6.3 TB/s of an in-order HBM sweep (MEASUREMENTS.md):
  gather   the windows' image and mask bytes read (4 ch cw) and the outputs written (3 R^2 + 4 R^2);
  paste    the windows' mask bytes, and per sample the generator's output (12 R^2) and the bytes read and written where A > 0 (6 per pixel).
Prints one JSON line per measurement; ``--out`` also writes them to a file.

``--holes N`` replaces the workload: N marks of about 200 x 150 scattered over each photograph, grouped on the device
(``inpaint.label_holes``, csrc/hole_label.hip) into one window per group.  Reported: the label sequence (kernels alone on buffers made
once, and the Python call) with the bytes it must move -- the mask read and the labels written, 5 per pixel -- beside the sweep, and
``scipy.ndimage.label`` of the same dilated masks on the host (one reading, one thread: scipy's labelling is serial); the owner launch;
gather and paste over the groups' windows (keyed) against the single window ``plan_window`` puts around all marks of a photograph."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shgan_amd  # noqa: E402,F401
from shgan_amd import _lib, inpaint, resize  # noqa: E402

DEV = 'cuda:0'
SWEEP_TBS = (6.0, 6.3)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                       # us per call


def torch_gather(imgs, masks, windows, R):
    real, mk = [], []
    for im, m, (y0, x0, ch, cw) in zip(imgs, masks, windows):
        crop = im[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1)[None].float()
        real.append(F.interpolate(crop, size=(R, R), mode='bicubic', antialias=True, align_corners=False).round_().clamp_(0, 255).to(torch.uint8))
        hole = (m[y0:y0 + ch, x0:x0 + cw] == 0).float()[None, None]
        mk.append(1.0 - F.adaptive_max_pool2d(hole, R))
    return torch.cat(real), torch.cat(mk)


def torch_paste(imgs, masks, windows, fake, k, feather):
    Fw = feather + 1
    outs = []
    for n, (im, m, (y0, x0, ch, cw)) in enumerate(zip(imgs, masks, windows)):
        hole = (m[y0:y0 + ch, x0:x0 + cw] == 0).float()[None, None]
        A, cur = hole.clone(), hole
        for _ in range(feather):
            cur = F.max_pool2d(cur, 3, 1, 1)
            A += cur
        A = A[0].permute(1, 2, 0)                                    # [ch, cw, 1]
        orig = im[y0:y0 + ch, x0:x0 + cw].float()
        for j in range(k):
            up = F.interpolate(fake[n * k + j][None], size=(ch, cw), mode='bicubic', align_corners=False)[0].permute(1, 2, 0)
            g = (up * 127.5 + 127.5).clamp_(0, 255)
            out = im.clone()
            out[y0:y0 + ch, x0:x0 + cw] = ((A * g + (Fw - A) * orig) / Fw).to(torch.uint8)
            outs.append(out)
    return outs


def holes_bench(a, report_into):
    import time
    B, H, W, R, feather, N = a.images, a.height, a.width, a.resolution, a.feather, a.holes
    rs = np.random.RandomState(1)
    imgs = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(B)]
    masks = []
    for _ in range(B):
        m = np.ones((H, W), np.uint8)
        for _ in range(N):
            bh, bw = 150 + int(rs.randint(-20, 21)), 200 + int(rs.randint(-20, 21))
            ya, xa = int(rs.randint(0, H - bh)), int(rs.randint(0, W - bw))
            m[ya:ya + bh, xa:xa + bw] = 0
        masks.append(m)
    packed, shapes = resize.pack_images(imgs)
    pm, moffs = inpaint.pack_masks(masks)
    shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
    packed, pm = packed.to(DEV), pm.to(DEV)
    lib = _lib.get_lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731
    px = int(pm.numel())

    def report(what, times, nbytes=None, **extra):
        for name, xs in times.items():
            xs = sorted(xs)
            rec = {'what': what, 'timing': name, 'us_median': round(xs[len(xs) // 2], 1), 'us_min': round(xs[0], 1), 'us_max': round(xs[-1], 1),
                   'rounds': len(xs), 'iters_per_round': a.iters}
            if name == 'kernel alone' and nbytes:
                tbs = nbytes / xs[len(xs) // 2] * 1e-6
                rec.update(bytes_to_move=int(nbytes), TB_per_s=round(tbs, 3), of_sweep=[round(tbs / s, 3) for s in SWEEP_TBS])
            rec.update(extra)
            report_into.append(rec)
            print(json.dumps(rec), flush=True)

    # the label sequence
    lbl = inpaint.label_holes(pm, shapes, feather)
    comps = inpaint.fetch_components(lbl)
    sh = torch.from_numpy(shapes.astype(np.int32).reshape(-1)).to(DEV)
    scratch = torch.empty(px, dtype=torch.int32, device=DEV)

    def label_kernels():
        _lib.check(lib.shg_hole_label_i32(ptr(pm), px, ptr(sh), B, H, W, feather + 1, lbl.max_components, ptr(lbl.labels), ptr(scratch),
                                          ptr(lbl.state[1:]), ptr(lbl.state), st), 'inpaint_bench')
    times = {'kernel alone': [], 'python call': []}
    for _ in range(a.rounds):
        times['kernel alone'].append(timed(label_kernels, 3, a.iters))
        times['python call'].append(timed(lambda: inpaint.label_holes(pm, shapes, feather), 3, a.iters))
    report(f'label_holes {B} x {H}x{W}, {N} marks each, feather {feather}', times, 5 * px, groups=int(comps.shape[0]))
    try:
        from scipy import ndimage
        t0 = time.perf_counter()
        n_host = 0
        for m in masks:
            D = ndimage.maximum_filter((m == 0).astype(np.uint8), size=2 * feather + 3, mode='constant', cval=0)
            n_host += ndimage.label(D, structure=np.ones((3, 3)))[1]
        host_us = (time.perf_counter() - t0) * 1e6
        rec = {'what': 'scipy.ndimage maximum_filter + label of the same masks on the host', 'timing': 'one reading, 1 thread', 'us': round(host_us, 1),
               'groups': int(n_host)}
        report_into.append(rec)
        print(json.dumps(rec), flush=True)
    except ImportError:
        print(json.dumps({'what': 'scipy is not installed: no host reading'}), flush=True)

    # the owner launch
    plan = inpaint.plan_windows(comps, shapes, R, 0.5, feather, max_windows=max(N, 1))
    owner = inpaint.owner_plane(lbl, pm, shapes, plan.table)
    tabd = torch.from_numpy(plan.table.astype(np.int32).reshape(-1)).to(DEV)

    def owner_kernels():
        _lib.check(lib.shg_hole_owner_u8(ptr(pm), px, ptr(sh), B, H, W, ptr(lbl.labels), ptr(tabd), plan.table.shape[0], ptr(scratch), ptr(owner), st),
                   'inpaint_bench')
    times = {'kernel alone': [], 'python call': []}
    for _ in range(a.rounds):
        times['kernel alone'].append(timed(owner_kernels, 3, a.iters))
        times['python call'].append(timed(lambda: inpaint.owner_plane(lbl, pm, shapes, plan.table), 3, a.iters))
    report(f'owner_plane {B} x {H}x{W}, {plan.table.shape[0]} groups', times, 10 * px)          # labels read twice, the mask read, the plane written

    # gather + paste: the groups' windows against one window per photograph
    one = np.array([inpaint.plan_window(m, R, 0.5, feather) for m in masks], np.int64)
    nw = plan.image.shape[0]
    wshapes = shapes[plan.image]
    fake_n = torch.rand(nw, 3, R, R, device=DEV) * 1.6 - 0.8
    fake_1 = torch.rand(B, 3, R, R, device=DEV) * 1.6 - 0.8
    out = packed.clone().view(1, -1)
    times = {'gather, per-group windows': [], 'gather, one window': [], 'paste (keyed), per-group windows': [], 'paste, one window': []}
    for _ in range(a.rounds):
        times['gather, per-group windows'].append(timed(lambda: inpaint.gather_windows(packed, pm, wshapes, plan.windows, R), 3, a.iters))
        times['gather, one window'].append(timed(lambda: inpaint.gather_windows(packed, pm, shapes, one, R), 3, a.iters))
        times['paste (keyed), per-group windows'].append(timed(lambda: inpaint.paste_back(packed, pm, wshapes, plan.windows, fake_n, feather=feather, out=out,
                                                                                          owner=owner, keys=plan.key), 3, a.iters))
        times['paste, one window'].append(timed(lambda: inpaint.paste_back(packed, pm, shapes, one, fake_1, feather=feather, out=out), 3, a.iters))
    report(f'python calls, {nw} windows of {int((plan.windows[:, 2] * plan.windows[:, 3]).sum())} px against {B} of {int((one[:, 2] * one[:, 3]).sum())} px',
           times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--height', type=int, default=2000)
    ap.add_argument('--width', type=int, default=3000)
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--feather', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--holes', type=int, default=0, help='N > 0: scatter N marks per image and time the hole-group path instead')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('inpaint_bench needs a GPU')
    if a.holes > 0:
        records = []
        holes_bench(a, records)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                for r in records:
                    fh.write(json.dumps(r) + '\n')
        return
    B, H, W, R, feather = a.images, a.height, a.width, a.resolution, a.feather
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(B)]
    masks = []
    for _ in range(B):
        bh, bw = int(0.35 * H + rs.randint(-20, 21)), int(0.30 * W + rs.randint(-20, 21))          # about 700 x 900 of 2000 x 3000
        ya, xa = int(rs.randint(0, H - bh)), int(rs.randint(0, W - bw))
        m = np.ones((H, W), np.uint8)
        m[ya:ya + bh, xa:xa + bw] = 0
        masks.append(m)
    windows = np.array([inpaint.plan_window(m, R, 0.5, feather) for m in masks], np.int64)
    packed, shapes = resize.pack_images(imgs)
    pm, moffs = inpaint.pack_masks(masks)
    shapes = np.concatenate([shapes.numpy().astype(np.int64), moffs[:, None]], axis=1)
    packed, pm = packed.to(DEV), pm.to(DEV)
    d_imgs, d_masks = [torch.from_numpy(x).to(DEV) for x in imgs], [torch.from_numpy(x).to(DEV) for x in masks]
    lib = _lib.get_lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731
    records = []
    win_px = int((windows[:, 2] * windows[:, 3]).sum())

    def report(what, k, times, nbytes):
        for name, xs in times.items():
            xs = sorted(xs)
            rec = {'what': what, 'K': k, 'timing': name, 'us_median': round(xs[len(xs) // 2], 1), 'us_min': round(xs[0], 1), 'us_max': round(xs[-1], 1),
                   'rounds': len(xs), 'iters_per_round': a.iters}
            if name == 'kernel alone':
                tbs = nbytes / xs[len(xs) // 2] * 1e-6
                rec.update(bytes_to_move=int(nbytes), TB_per_s=round(tbs, 3), of_sweep=[round(tbs / s, 3) for s in SWEEP_TBS])
            records.append(rec)
            print(json.dumps(rec), flush=True)

    # gather
    table, chunks, bands, lds = inpaint.build_gather_table(shapes, windows, R)
    tab = torch.from_numpy(table).to(DEV)
    real, mk = inpaint.gather_windows(packed, pm, shapes, windows, R)

    def gather_kernel():
        _lib.check(lib.shg_inpaint_gather_u8(ptr(packed), packed.numel(), ptr(pm), pm.numel(), ptr(tab), tab.numel(), ptr(real), ptr(mk), B, R, chunks,
                                             bands, lds, st), 'inpaint_bench')
    times = {'kernel alone': [], 'python call': [], 'torch operators': []}
    for _ in range(a.rounds):                                         # the three alternate within a round
        times['kernel alone'].append(timed(gather_kernel, 3, a.iters))
        times['python call'].append(timed(lambda: inpaint.gather_windows(packed, pm, shapes, windows, R), 3, a.iters))
        times['torch operators'].append(timed(lambda: torch_gather(d_imgs, d_masks, windows.tolist(), R), 2, max(a.iters // 4, 2)))
    report(f'gather_windows {B} x {H}x{W} -> {R}^2', 1, times, 4 * win_px + B * 7 * R * R)

    # paste
    for k in (1, 4):
        fake = (torch.rand(B * k, 3, R, R, device=DEV) * 1.6 - 0.8)
        alpha = torch.zeros(pm.numel(), dtype=torch.uint8, device=DEV)
        out = inpaint.paste_back(packed, pm, shapes, windows, fake, k=k, feather=feather, alpha_out=alpha)
        active = int((alpha > 0).sum().item())
        table, chunks, bands, lds = inpaint.build_paste_table(shapes, windows, R, feather)
        tab = torch.from_numpy(table).to(DEV)

        def paste_kernel():                                           # (blends into the same buffer again: the same work per launch)
            _lib.check(lib.shg_inpaint_paste_u8(ptr(out), packed.numel(), ptr(pm), pm.numel(), ptr(tab), tab.numel(), ptr(fake), None, B, k, R, feather,
                                                chunks, bands, lds, st), 'inpaint_bench')
        times = {'kernel alone': [], 'python call': [], 'torch operators': []}
        for _ in range(a.rounds):
            times['kernel alone'].append(timed(paste_kernel, 3, a.iters))
            times['python call'].append(timed(lambda: inpaint.paste_back(packed, pm, shapes, windows, fake, k=k, feather=feather, out=out), 3, a.iters))
            times['torch operators'].append(timed(lambda: torch_paste(d_imgs, d_masks, windows.tolist(), fake, k, feather), 1, max(a.iters // 10, 2)))
        report(f'paste_back {B} x {H}x{W}, window px {win_px}, active px {active}, feather {feather}', k, times,
               win_px + k * (B * 12 * R * R + 6 * active))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for r in records:
                fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
