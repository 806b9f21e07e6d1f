#!/usr/bin/env python3
"""Per-stage time of the Spectral Hint Unit at input sizes 32, 64 and 128 (C = 32, batch 16, pyramid down to 4): rfft2 + shift, the
fused spectral stage, split + irfft2 -- each next to the same stage done with torch.fft / torch ops on the device.

Method: device events around a window of back-to-back calls that lasts at least ``--window`` seconds after a warm-up of every shape;
each figure is the median of ``--repeats`` windows, HIP and torch windows alternating, with the spread (min .. max) beside it.  The
times include the host's launch path of the Python wrappers (one launch per call), as a user of ``kernels.shu_*`` pays it.

``--parent-lib PATH`` also times the shipped 64 x 64 entry points of another build of libshgan_hip.so (the parent commit's) in the
same run, alternating with this build's: the 64 row is the same code and must agree within the spread.

Usage:  python tools/shu_geometry_bench.py [--parent-lib PATH] [--json OUT]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import shgan_amd  # noqa: E402,F401
from shgan_amd import kernels as kk  # noqa: E402
from shgan_amd.model_zoo import shgan  # noqa: E402

N, C = 16, 32


def window(fn, seconds):
    """-> microseconds per call over a window of at least ``seconds``."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    while True:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms / reps * 1e3
        reps = int(reps * max(2.0, 1.2 * seconds * 1e3 / max(ms, 1e-3)))


def compare(fns, seconds, repeats):
    """fns: {label: callable}; windows alternate between the labels -> {label: (median, min, max)} in microseconds."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            got[k].append(window(fn, seconds))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def torch_split(s, gauss, size):
    ch = s.shape[1] // 2
    sp = torch.complex(s[:, :ch], s[:, ch:])
    out = []
    for g in gauss:
        r = g.shape[0]
        t = sp[:, :, size // 2 - r // 2: size // 2 + r // 2, 0: r // 2 + 1] * g
        out.append(torch.fft.irfftn(torch.roll(t, -(r - r // 2 - 1), dims=2), dim=(2, 3), norm='forward'))
    return out


def parent_calls(path, x, t, w0p, b0, w1p, cw, s, gauss, outs):
    """The shipped 64 x 64 entry points of another build, called on the same buffers."""
    lib = ctypes.CDLL(path)
    P = ctypes.c_void_p
    stream = P(torch.cuda.current_stream().cuda_stream)
    lib.shg_shu_rfft2_shift_f32.argtypes = [P, ctypes.c_long, P, ctypes.c_int, ctypes.c_int, P]
    lib.shg_shu_spectral_f32.argtypes = [P] * 6 + [ctypes.c_int] * 4 + [P]
    lib.shg_shu_split_irfft2_f32.argtypes = [P, P, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(ctypes.c_long)] + [ctypes.c_int] * 4 + [P]
    g_arr = (P * 5)(*[g.data_ptr() for g in gauss])
    o_arr = (P * 5)(*[o.data_ptr() for o in outs])
    s_arr = (ctypes.c_long * 5)(*[o.stride(0) for o in outs])
    tp, sp_ = torch.empty_like(t), torch.empty_like(s)
    return dict(
        rfft2=lambda: lib.shg_shu_rfft2_shift_f32(x.data_ptr(), x.stride(0), tp.data_ptr(), N, C, stream),
        spectral=lambda: lib.shg_shu_spectral_f32(t.data_ptr(), w0p.data_ptr(), b0.data_ptr(), w1p.data_ptr(), cw.data_ptr(), sp_.data_ptr(), N, 2 * C,
                                                  64 * 33, cw.shape[0], stream),
        split=lambda: lib.shg_shu_split_irfft2_f32(s.data_ptr(), None, g_arr, o_arr, s_arr, N, C, 1, 0, stream))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('shu_geometry_bench: no GPU -- times are measured on the device or not at all')
    rows = []
    for size in (32, 64, 128):
        torch.manual_seed(size)
        shu = shgan.SHU(C, C, [2, 3], 'piecewise_linear', input_res=size, lowest_res=4, tail_sigma_mult=3).cuda().eval()
        with torch.no_grad():
            shu.conv0.bias.normal_(0, 0.2)
            x = torch.randn(N, C, size, size, device='cuda')
            w0p, b0, w1p = shu._packed()
            gauss = [getattr(shu, f'_gauss{r}') for r in shu.reslist]
            t = kk.shu_rfft2_shift(x)
            s = kk.shu_spectral(t, w0p, b0, w1p, shu._cw)
            outs = [torch.empty(N, C, r, r, device='cuda') for r in shu.reslist]
            w0 = (shu.conv0.weight * shu.conv0.weight_gain).contiguous()
            w1 = shu.df1.weight.t().contiguous()[:, :, None, None]
            cw = shu._cw

            def torch_spectral():
                y = torch.nn.functional.conv2d(torch.relu(torch.nn.functional.conv2d(t, w0, b0)), w1)
                return (y.view(N, 2 * C, cw.shape[0], size, size // 2 + 1) * cw).sum(2)

            def torch_rfft2():
                sp = torch.roll(torch.fft.rfftn(x, dim=(2, 3), norm='forward'), size // 2 - 1, dims=2)
                return torch.cat([sp.real, sp.imag], dim=1)

            stages = dict(
                rfft2=dict(hip=lambda: kk.shu_rfft2_shift(x), torch=torch_rfft2),
                spectral=dict(hip=lambda: kk.shu_spectral(t, w0p, b0, w1p, cw), torch=torch_spectral),
                split=dict(hip=lambda: kk.shu_split_irfft2(s, None, gauss, outs, False), torch=lambda: torch_split(s, gauss, size)))
            if a.parent_lib and size == 64:
                for k, fn in parent_calls(a.parent_lib, x, t, w0p, b0, w1p, cw, s, gauss, outs).items():
                    stages[k]['parent'] = fn
            for stage, fns in stages.items():
                for label, (med, lo, hi) in compare(fns, a.window, a.repeats).items():
                    rows.append(dict(size=size, stage=stage, impl=label, us=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2)))
                    print(f'size {size:4d}  {stage:9s} {label:7s} {med:9.1f} us   ({lo:.1f} .. {hi:.1f})', flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(dict(batch=N, channels=C, lowest_res=4, window_s=a.window, repeats=a.repeats, device=torch.cuda.get_device_name(0),
                           rows=rows), fh, indent=1)


if __name__ == '__main__':
    main()
