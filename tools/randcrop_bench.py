"""The random-scale crop launch (resize.randcrop_bicubic, csrc/randcrop.hip) timed with device events after a warm-up, at the two training
shapes: 512^2 x 8 windows from 600 x 800 ragged sources (DTD-like: the formatter's draws for that size) and 256^2 x 32 windows from planar
256^2 sources (Places2 'adv': the loader's resize comes first and is not timed here).  Bytes moved = 12 s^2 per window written plus the
window's footprint of source bytes read (the rows and columns its taps touch, computed from the drawn parameters), over the time per
launch, against the 6.3 TB/s copy ceiling.  Two timings per shape: the kernel alone (the C entry point in a loop on a descriptor already
on the device: back-to-back launches, so the figure is the larger of the kernel's time and the host's launch rate) and the Python call
as a training step pays it (descriptor pinned and uploaded per call).
Prints one JSON line per measurement; ``--out`` also writes them to a file."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shgan_amd  # noqa: E402,F401
from shgan_amd import _lib, datasets, resize as rz  # noqa: E402

DEV = 'cuda:0'
COPY_CEILING_TBS = 6.3


def footprint_bytes(h, w, s, params):
    """source bytes the window's taps touch: (rows) x (columns) x 3"""
    nh, nw, ch, cw = (int(v) for v in params[:4])
    iy, _ = rz._cubic_axis(h, nh, np.array([ch, ch + s - 1]))
    ix, _ = rz._cubic_axis(w, nw, np.array([cw, cw + s - 1]))
    rows = min(int(iy[1]) + 3, h - 1) - max(int(iy[0]), 0) + 1
    cols = min(int(ix[1]) + 3, w - 1) - max(int(ix[0]), 0) + 1
    return rows * cols * 3


def block(what, src, shapes, hw, s, params, iters, check_imgs, records):
    B = len(params)
    for _ in range(10):
        rz.randcrop_bicubic(src, shapes, s, params)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = rz.randcrop_bicubic(src, shapes, s, params)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3

    # the kernel alone: same launch, descriptor and output buffers fixed
    planar = src.ndim == 4
    shp = shapes if shapes is not None else np.stack([np.full(B, src.shape[2]), np.full(B, src.shape[3]),
                                                       np.arange(B) * 3 * src.shape[2] * src.shape[3]], axis=1)
    desc = rz.randcrop_desc(shp, params)
    dd, lut = torch.from_numpy(desc).to(DEV), rz._randcrop_lut(torch.device(DEV))
    fn = _lib.get_lib().shg_randcrop_bicubic_planar_f32 if planar else _lib.get_lib().shg_randcrop_bicubic_ragged_f32
    flat = src.contiguous().view(-1)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (ctypes.c_void_p(flat.data_ptr()), flat.numel(), desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.c_void_p(dd.data_ptr()),
            ctypes.c_void_p(lut.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, s, st)
    for _ in range(10):
        _lib.check(fn(*args), 'randcrop_bench')
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn(*args)
    e1.record()
    torch.cuda.synchronize()
    us_kernel = e0.elapsed_time(e1) / iters * 1e3
    worst = max(float(np.abs(out[i].cpu().numpy() - rz.randcrop_reference(check_imgs[i], s, params[i])).max()) for i in (0, B - 1))
    nbytes = B * 12 * s * s + sum(footprint_bytes(h, w, s, p) for (h, w), p in zip(hw, params))
    rec = {'what': what + ' (device events)', 'B': B, 's': s, 'iters': iters, 'us_kernel_back_to_back': round(us_kernel, 2),
           'us_python_call_with_descriptor_upload': round(us, 2), 'bytes': int(nbytes), 'TB_per_s': round(nbytes / us_kernel * 1e-6, 3),
           'of_copy_ceiling': round(nbytes / us_kernel * 1e-6 / COPY_CEILING_TBS, 3),
           'max_abs_diff_vs_host_reference_sampled': worst}
    records.append(rec)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('randcrop_bench needs a GPU')
    records = []
    rs = np.random.RandomState(0)

    np.random.seed(1)
    imgs = [rs.randint(0, 256, size=(600, 800, 3)).astype(np.uint8) for _ in range(8)]
    params = [datasets.draw_scale_crop(600, 800, 512, flips=True) for _ in imgs]
    packed, shapes = rz.pack_images(imgs)
    block('randcrop_bicubic ragged, 600x800 sources -> 512^2 x 8', packed.to(DEV), shapes, [(600, 800)] * 8, 512, params, a.iters, imgs, records)

    planar = rs.randint(0, 256, size=(32, 3, 256, 256)).astype(np.uint8)
    params = [datasets.draw_scale_crop(256, 256, 256, flips=False) for _ in range(32)]
    hwc = [np.ascontiguousarray(p.transpose(1, 2, 0)) for p in planar]
    block('randcrop_bicubic planar, 256^2 sources -> 256^2 x 32', torch.from_numpy(planar).to(DEV), None, [(256, 256)] * 32, 256, params, a.iters,
          hwc, records)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for r in records:
                fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
