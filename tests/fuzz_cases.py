"""Test helper: the random-shape case generators, one per family, shared by the bounded suite (tests/test_gpu_fuzz.py: fixed seeds, one
test per case) and the long sweeps (tools/fuzz.py FAMILY [cases] [first_seed] [--full]).  Nothing here is shipped.

``_case_<family>(seed)`` draws one case from its own RNG stream, runs it on cuda:0 and returns a list of (what, error, bound,
description); an empty list means the draw is not a valid problem.  So a failing seed of either user reproduces alone in the other.
References are float64; the bounds are those of the sweeps these families were first written as (tools/ARCHIVE.md).  The families of
``FULL`` take ``full=True``: by default their largest choices are trimmed so that the float64 references of the suite stay cheap,
``full=True`` draws from the untrimmed lists and ranges (other cases than the same seed gives by default)."""
import random

import numpy as np
import torch
import torch.nn.functional as F

DEV = 'cuda:0'
CL = torch.channels_last


def _mods():
    import shgan_amd  # noqa: F401
    from shgan_amd import _lib, kernels, kernels_f16
    from oracle import shgan_oracle as orc
    return kernels, kernels_f16, _lib, orc


def rel(a, b):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.from_numpy(np.asarray(b, np.float64))
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


# ------------------------------------------------------------------------------------------------
# ops: same / stride-2 / transposed 3x3 convolutions with the layer tail, and 4x4 FIR, against the oracle (bound 2e-5)
# ------------------------------------------------------------------------------------------------

def _case_ops(seed, full=False):
    kk, _, _, orc = _mods()
    rs = np.random.RandomState(seed)
    kind = rs.choice(['same', 'down', 'up', 'fir'])
    n = int(rs.choice([1, 2, 3, 5] if full else [1, 2, 3]))
    ci = int(rs.choice([3, 8, 9, 16, 24, 40, 64, 72, 130]))
    co = int(rs.choice([3, 16, 33, 64, 70, 128, 192]))
    h = int(rs.choice([4, 7, 8, 16, 31, 32, 33, 40, 64, 68]))
    w = int(rs.choice([4, 8, 12, 16, 31, 32, 36, 44, 64, 65]))
    if kind == 'same' and rs.rand() < 0.4:      # wide images: the 8 x 64 and 4 x 128 tile shapes of the F(4x4) kernel
        w, h = int(rs.choice([128, 132, 200, 256, 260])), int(rs.choice([8, 12, 20, 33]))
        ci, co, n = int(rs.choice([8, 16, 24])), int(rs.choice([16, 64, 70])), int(rs.choice([1, 2]))
    while not full and 9 * n * ci * co * h * w > 2e8:    # (keeps the float64 reference cheap)
        if n > 1:
            n -= 1
        else:
            h = max(4, h // 2)
    x = torch.from_numpy(rs.standard_normal((n, ci, h, w)).astype(np.float32))
    if kind == 'fir':
        f = torch.from_numpy(rs.rand(4, 4).astype(np.float32))
        pad = [int(v) for v in rs.randint(0, 4, 4)]
        up, down = int(rs.choice([1, 2])), int(rs.choice([1, 2]))
        flip, gain = bool(rs.randint(2)), float(rs.choice([1.0, 4.0, 0.37]))
        ref = orc.upfirdn2d(x.double(), f.double(), up=up, down=down, padding=pad, flip_filter=flip, gain=gain)
        y = kk.upfirdn2d(x.to(DEV), f.to(DEV), upx=up, upy=up, downx=down, downy=down, padx0=pad[0], padx1=pad[1],
                         pady0=pad[2], pady1=pad[3], flip=flip, gain=gain)
        desc = f'fir n{n} c{ci} {h}x{w} up{up} down{down} pad{pad} flip{flip} gain{gain}'
    else:
        wt = torch.from_numpy(rs.standard_normal((co, ci, 3, 3)).astype(np.float32))
        mod = bool(rs.randint(2))
        s_in = torch.from_numpy(rs.rand(n, ci).astype(np.float32) + 0.5) if mod else None
        s_out = torch.from_numpy(rs.rand(n, co).astype(np.float32) + 0.5) if mod else None
        bias = torch.from_numpy(rs.standard_normal(co).astype(np.float32))
        flip = bool(rs.randint(2)) and kind != 'up'
        wref = (wt.flip([2, 3]) if flip else wt).double()
        xin = x.double() * s_in.double()[:, :, None, None] if mod else x.double()
        if kind == 'same':
            ref = F.conv2d(xin, wref * 0.1, padding=1); mode, pad = 0, 1
        elif kind == 'down':
            ref = F.conv2d(xin, wref * 0.1, stride=2); mode, pad = 1, 0
        else:
            ref = F.conv_transpose2d(xin, (wt.double() * 0.1).transpose(0, 1), stride=2); mode, pad = 2, 0
        if mod:
            ref = ref * s_out.double()[:, :, None, None]
        ref = orc.lrelu_agc(ref + bias.double().view(1, -1, 1, 1), gain=0.7)
        pw = kk.conv_weight_prep(wt.to(DEV), gain=0.1, flip=flip)
        y = kk.conv2d(x.to(DEV), pw, mode=mode, pad=pad, in_scale=None if s_in is None else s_in.to(DEV),
                      out_scale=None if s_out is None else s_out.to(DEV), bias=bias.to(DEV), act=True, gain=0.7)
        desc = f'{kind} n{n} {ci}->{co} {h}x{w} mod{mod} flip{flip}'
    assert tuple(y.shape) == tuple(ref.shape), (desc, tuple(y.shape), tuple(ref.shape))
    return [(kind, rel(y, ref), 2e-5, desc)]


# ------------------------------------------------------------------------------------------------
# fir_march: the row-marching separable FIR kernels (pad-2, polyphase planes, x2 down / up, FIR from phase planes + tail), bound 2e-5;
# the polyphase planes are zero (below 1e-6) wherever the reference is: outside the image, up to the drawn pitch
# ------------------------------------------------------------------------------------------------

def _case_fir_march(seed):
    kk, _, _lib, orc = _mods()
    lib = _lib.get_lib()
    rs = np.random.RandomState(seed)
    out = []

    def taps():
        if rs.randint(2):
            return orc.setup_filter([1, 3, 3, 1])
        while True:          # exactly representable taps: the outer product stays rank 1 in fp32
            a, b = rs.randint(-8, 9, 4) / 8.0, rs.randint(-8, 9, 4) / 4.0
            if abs(a.sum() * b.sum()) > 0.1:
                return torch.from_numpy(np.outer(a, b).astype(np.float32))

    kind = rs.choice(['pad2', 'planes', 'dn2', 'up2', 'upfir'])
    n, c = int(rs.choice([1, 2, 3, 7])), int(rs.choice([1, 2, 3, 5, 13, 37]))
    f = taps()
    flip, gain = bool(rs.randint(2)), float(rs.choice([1.0, 4.0, 0.37]))
    if kind in ('pad2', 'planes', 'dn2'):
        w = int(rs.choice([8, 16, 32, 64, 128, 256, 512]))
        h = int(rs.choice([2, 4, 6, 10, 16, 34, 64, 130])) if kind != 'pad2' else int(rs.choice([2, 3, 5, 9, 16, 33, 64, 131]))
        if w >= 256:
            n, c = min(n, 2), min(c, 5)
        desc = f'{kind} n{n} c{c} {h}x{w} flip{flip} gain{gain}'
        x = torch.from_numpy(rs.standard_normal((n, c, h, w)).astype(np.float32))
        if kind == 'dn2':
            ref = orc.upfirdn2d(x.double(), f.double(), down=2, padding=[1, 1, 1, 1], flip_filter=flip, gain=gain)
            assert lib.shg_fir_resample2_sep_supported(h, w, 1)
            y = kk.upfirdn2d(x.to(DEV), f.to(DEV), downx=2, downy=2, padx0=1, padx1=1, pady0=1, pady1=1, flip=flip, gain=gain)
        else:
            ref = orc.upfirdn2d(x.double(), f.double(), padding=[2, 2, 2, 2], flip_filter=flip, gain=gain)
            if kind == 'pad2':
                assert lib.shg_fir_pad2_sep_supported(h, w, 0)
                y = kk.upfirdn2d(x.to(DEV), f.to(DEV), padx0=2, padx1=2, pady0=2, pady1=2, flip=flip, gain=gain)
            else:
                pp = (w // 2 + 1 + 3) // 4 * 4 + 4 * int(rs.choice([0, 0, 1, 3, 7]))
                desc += f' pitch{pp}'
                assert lib.shg_fir_pad2_sep_supported(h, w, pp)
                xp = torch.full((4, n, c, h // 2 + 1, pp), float('nan'), device=DEV)
                xd, fd = x.to(DEV), f.to(DEV)           # (kept alive across the raw C call)
                kk.check(lib.shg_fir_pad2_sep_f32(kk._ptr(xd), kk.sep_taps(fd), kk._ptr(xp), n, c, h, w, pp, int(flip), gain, None), 'pad2')
                torch.cuda.synchronize()
                full = torch.zeros(n, c, 2 * (h // 2 + 1), 2 * pp, dtype=torch.float64)
                full[:, :, :h + 1, :w + 1] = ref
                got = xp.cpu()
                assert not torch.isnan(got).any(), (desc, 'unwritten plane entries')
                y = torch.zeros_like(full)
                for a in range(2):
                    for b in range(2):
                        y[:, :, a::2, b::2] = got[a * 2 + b].double()
                ref = full
                out.append(('planes where ref is 0', float(y[ref == 0].abs().max()) if (ref == 0).any() else 0.0, 1e-6, desc))
    elif kind == 'up2':
        w = int(rs.choice([4, 8, 16, 32, 64, 128, 256])); h = int(rs.choice([1, 2, 3, 8, 17, 64, 100]))
        if w >= 128:
            n, c = min(n, 2), min(c, 5)
        desc = f'{kind} n{n} c{c} {h}x{w} flip{flip} gain{gain}'
        x = torch.from_numpy(rs.standard_normal((n, c, h, w)).astype(np.float32))
        ref = orc.upfirdn2d(x.double(), f.double(), up=2, padding=[2, 1, 2, 1], flip_filter=flip, gain=gain)
        assert lib.shg_fir_resample2_sep_supported(h, w, 2)
        y = kk.upfirdn2d(x.to(DEV), f.to(DEV), upx=2, upy=2, padx0=2, padx1=1, pady0=2, pady1=1, flip=flip, gain=gain)
    else:
        w = int(rs.choice([4, 8, 16, 32, 64, 128, 256])); h = int(rs.choice([1, 2, 3, 8, 17, 64, 100]))
        if w >= 128:
            n, c = min(n, 2), min(c, 5)
        mid = torch.from_numpy(rs.standard_normal((4, n, c, h + 1, w + 1)).astype(np.float32))
        full = torch.zeros(n, c, 2 * h + 1, 2 * w + 1, dtype=torch.float64)
        for a in range(2):
            for b in range(2):
                full[:, :, a::2, b::2] = mid[a * 2 + b][:, :, :h + 1 - a, :w + 1 - b].double()
        ref = orc.upfirdn2d(full, f.double(), padding=[1, 1, 1, 1], flip_filter=flip, gain=4.0)
        kw = {}
        if rs.randint(2):
            kw['scale'] = torch.from_numpy(rs.rand(n * c).astype(np.float32) + 0.5); ref = ref * kw['scale'].double().view(n, c, 1, 1)
        if rs.randint(2):
            per = bool(rs.randint(2)) and n > 1
            kw['noise'] = torch.from_numpy(rs.standard_normal((n if per else 1, 1, 2 * h, 2 * w)).astype(np.float32))
            ref = ref + kw['noise'].double() * np.float32(0.3)
        if rs.randint(2):
            kw['bias'] = torch.from_numpy(rs.standard_normal(c).astype(np.float32)); ref = ref + kw['bias'].double().view(1, c, 1, 1)
        act = bool(rs.randint(2))
        if act:
            ref = orc.lrelu_agc(ref, gain=0.8)
        if rs.randint(2):
            kw['residual'] = torch.from_numpy(rs.standard_normal((n, c, 2 * h, 2 * w)).astype(np.float32)); ref = ref + kw['residual'].double()
        desc = f'{kind} n{n} c{c} {h}x{w} flip{flip} act{act} tail{sorted(kw)}'
        assert lib.shg_upfir_planar_sep_supported(h, w)
        y = kk.upfir_planar(mid.to(DEV), f.to(DEV), noise_strength=0.3, act=act, gain=0.8, flip=flip, **{k: v.to(DEV) for k, v in kw.items()})
    assert tuple(y.shape) == tuple(ref.shape), (desc, tuple(y.shape), tuple(ref.shape))
    return [(kind, rel(y, ref), 2e-5, desc)] + out


# ------------------------------------------------------------------------------------------------
# round4: fp16 relayout (exact), style factors and their first-order backward (vs float64 autograd, 5e-5), weight packs (exact)
# ------------------------------------------------------------------------------------------------

def _case_round4(seed):
    _, kf, _, _ = _mods()
    from shgan_amd.model_zoo import stylegan as sg
    rnd = random.Random(seed)
    torch.manual_seed(seed)
    out = []
    n, c, h, w = rnd.randint(1, 5), rnd.choice([1, 3, 4, 8, 16, 24, 40, 64, 72, 128, 520]), rnd.randint(1, 70), rnd.randint(1, 70)
    x = torch.randn(n, c, h, w, device=DEV) * 10 ** rnd.uniform(-3, 5)
    if kf.relayout_supported(x):
        ref = x.to(dtype=torch.float16, memory_format=CL)
        a, b = kf.relayout(x), kf.relayout(ref)
        out.append(('relayout', 0.0 if (torch.equal(a, ref) and torch.equal(b, ref.float())) else 1.0, 0.5, f'{(n, c, h, w)} exact'))
    N, I, O, half = rnd.randint(1, 16), rnd.choice([8, 32, 64, 100, 128, 256, 512]), rnd.choice([3, 8, 64, 70, 128, 512]), rnd.random() < 0.5
    if N * I <= 8192:
        s64 = torch.randn(N, I, dtype=torch.float64, device=DEV) + rnd.uniform(-1, 1)
        w64 = torch.rand(O, I, dtype=torch.float64, device=DEV) * 0.02
        ga, gb = torch.randn(N, I, dtype=torch.float64, device=DEV), torch.randn(N, O, dtype=torch.float64, device=DEV)

        def ref_fn(s, wq):
            if half:
                s = s / s.norm(float('inf'), dim=1, keepdim=True)
            s = s * s.square().mean().rsqrt()
            return s, (s.square().matmul(wq.t()) + 1e-8).rsqrt()
        res = []
        for fn, dt in ((ref_fn, torch.float64), (lambda s, wq: sg._StyleFactorsFn.apply(s, wq, half), torch.float32)):
            s = s64.to(dt).clone().requires_grad_(True)
            wq = w64.to(dt).clone().requires_grad_(True)
            with torch.enable_grad():
                sn, d = fn(s, wq)
                gs, gw = torch.autograd.grad((sn * ga.to(dt)).sum() + (d * gb.to(dt)).sum(), [s, wq])
            res.append((sn.detach(), d.detach(), gs, gw))
        for name, u, v in zip(('sn', 'd', 'gs', 'gw'), res[1], res[0]):
            out.append((f'style_factors {name}', rel(u, v), 5e-5, f'N{N} I{I} O{O} half{half}'))
    o, i, k = rnd.choice([8, 24, 32, 64, 96, 128]), rnd.choice([3, 4, 16, 40, 64, 128]), rnd.choice([1, 3])
    wt = torch.randn(o, i, k, k, device=DEV).half()
    old = kf.PACK_DIRECT
    try:
        for tr in (False, True):
            for fl in (False, True):
                src = wt.transpose(0, 1).contiguous() if tr else wt
                kf.PACK_DIRECT = True
                p1 = kf.pack_weight(src, transposed=tr, flip=fl)
                kf.PACK_DIRECT = False
                p2 = kf.pack_weight(src, transposed=tr, flip=fl)
                out.append(('pack', 0.0 if torch.equal(p1.wp, p2.wp) else 1.0, 0.5, f'o{o} i{i} k{k} transposed{tr} flip{fl} exact'))
    finally:
        kf.PACK_DIRECT = old
    return out


# ------------------------------------------------------------------------------------------------
# round5: Winograd-domain weight gradient (2e-5), fp16 ring and merged-phase transposed kernels (bit-equal to the gather
# kernels; 2e-3 against float64), the modulation tail's second product (2e-5 float32, 4e-3 / 2e-3 fp16)
# ------------------------------------------------------------------------------------------------

def _case_round5(seed, full=False):
    kk, kf, _lib, _ = _mods()
    lib = _lib.get_lib()
    rnd = random.Random(seed)
    torch.manual_seed(seed)
    out = []
    wg_n, wg_h, wg_w4, ring_hw, up_hw = (6, 70, 18, 80, 50) if full else (4, 40, 12, 64, 40)      # largest batch / extents drawn

    def routes(fn):
        old = lib.shg_conv2d_f16_set_routes(7)
        try:
            a = fn()
            lib.shg_conv2d_f16_set_routes(0)
            b = fn()
        finally:
            lib.shg_conv2d_f16_set_routes(old)
        torch.cuda.synchronize()
        return a, b

    n, ci, co = rnd.randint(1, wg_n), rnd.choice([1, 3, 8, 20, 32, 33, 64, 70, 96, 130]), rnd.choice([2, 8, 16, 31, 64, 65, 100, 128])
    h, w = rnd.randint(4, wg_h), 4 * rnd.randint(1, wg_w4)
    x, g = torch.randn(n, ci, h, w, device=DEV), torch.randn(n, co, h, w, device=DEV)
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 3, 3), g.double(), stride=1, padding=1)      # (float64 on the device)
    out.append(('wgrad_wino', rel(kk.conv2d_wgrad(x, g, 3, 3, 1, 1), ref), 2e-5, f'n{n} {ci}->{co} {h}x{w}'))
    # ring kernel (+ tail) against the gather kernel
    n, i, o = rnd.randint(1, 4), 32 * rnd.randint(1, 6), 8 * rnd.randint(1, 20)
    h, w = rnd.randint(3, ring_hw), rnd.randint(3, ring_hw)
    xh = torch.randn(n, i, h, w, device=DEV).half().to(memory_format=CL)
    wt = (torch.randn(o, i, 3, 3, device=DEV) / (i * 9) ** 0.5).half()
    kw, b = {}, (torch.randn(o, device=DEV) if rnd.random() < 0.6 else None)
    if rnd.random() < 0.7:
        kw.update(act=rnd.random() < 0.7, gain=rnd.choice([1.0, 0.5, 2 ** 0.5]), clamp=rnd.choice([256.0, 1.0, -1.0]))
        if rnd.random() < 0.5:
            kw['out_scale'] = torch.rand(n, o, device=DEV) + 0.5
        if rnd.random() < 0.5 and w % 4 == 0:
            kw['noise'], kw['noise_strength'] = (torch.randn(h, w, device=DEV) if rnd.random() < 0.5 else torch.randn(n, 1, h, w, device=DEV)), 0.3
    a, c = routes(lambda: kf.conv2d(xh, wt, b, 1, 1, **kw))
    desc = f'n{n} {i}->{o} {h}x{w} tail{sorted(kw)}'
    out.append(('ring vs gather', 0.0 if torch.equal(a, c) else 1.0, 0.5, desc + ' exact'))
    if not kw:
        ref = F.conv2d(xh.double(), wt.double(), None if b is None else b.double(), 1, 1)
        out.append(('ring vs float64', rel(a, ref), 2e-3, desc))
    # merged-phase transposed kernel
    n, i, o = rnd.randint(1, 4), 32 * rnd.randint(1, 6), 8 * rnd.randint(1, 16)
    h, w, pad = rnd.randint(1, up_hw), rnd.randint(1, up_hw), rnd.choice([0, 1])
    out_hw = None if rnd.random() < 0.6 else (2 * h + rnd.randint(-1, 2), 2 * w + rnd.randint(-1, 2))
    if out_hw is None and (2 * h + 1 - 2 * pad < 1 or 2 * w + 1 - 2 * pad < 1):
        pad = 0
    xh = torch.randn(n, i, h, w, device=DEV).half().to(memory_format=CL)
    wt = (torch.randn(i, o, 3, 3, device=DEV) / (i * 9 / 4) ** 0.5).half()
    s = (torch.rand(n, i, device=DEV) + 0.5) if rnd.random() < 0.5 else None
    a, c = routes(lambda: kf.conv_transpose2d(xh, wt, None, pad, out_hw, in_scale=s))
    desc = f'n{n} {i}->{o} {h}x{w} pad{pad} out{out_hw} in_scale{s is not None}'
    out.append(('upring vs per-phase', 0.0 if torch.equal(a, c) else 1.0, 0.5, desc + ' exact'))
    xs = xh.double() if s is None else (xh * s.half().reshape(n, i, 1, 1)).double()
    ref = F.conv_transpose2d(xs.cpu(), wt.double().cpu(), stride=2, padding=0)
    oh, ow = out_hw if out_hw else (ref.shape[2] - 2 * pad, ref.shape[3] - 2 * pad)
    full = torch.zeros(n, o, pad + oh + 4, pad + ow + 4, dtype=torch.float64)
    full[:, :, :ref.shape[2], :ref.shape[3]] = ref
    out.append(('upring vs float64', rel(a, full[:, :, pad:pad + oh, pad:pad + ow]), 2e-3, desc))
    # modulation tail backward with the second product: A'(y) (gy d + u e) and sum_hw gz t
    n, c8, hw = rnd.randint(1, 4), rnd.choice([1, 2, 4, 8]), 4 * rnd.randint(1, 60)
    c, hh = 8 * c8, rnd.choice([1, 2, 4])
    while hw % hh:
        hh //= 2
    shape = (n, c, hh, hw // hh)
    for half in (False, True):
        dt = torch.float16 if half else torch.float32

        def mk():
            t = torch.randn(shape, device=DEV)
            return t.to(dt).contiguous(memory_format=CL) if half else t
        gy, y, t, u = mk(), mk(), mk(), mk()
        d, ee = torch.rand(n, c, device=DEV) + 0.5, torch.randn(n, c, device=DEV)
        act = rnd.random() < 0.7
        mod = kf if half else kk
        gt, s1, _, _ = mod.modtail_backward(gy, y, t, d, want_sums=True, want_noise=False, act=act, gain=1.0, clamp=1.5, u=u, e=ee)
        yd = y.double()
        slope = torch.where(yd.abs() >= 1.5, torch.zeros_like(yd), torch.where(yd > 0, torch.full_like(yd, 2 ** 0.5), torch.full_like(yd, 0.2 * 2 ** 0.5))) \
            if act else torch.ones_like(yd)
        gz = gy.double() * slope
        ref_gt = gz * d.double().reshape(n, c, 1, 1) + u.double() * slope * ee.double().reshape(n, c, 1, 1)
        ref_s1 = (gz * t.double()).sum([2, 3])
        desc = f'{shape} half{half} act{act}'
        out.append(('modtail gt', rel(gt, ref_gt), 4e-3 if half else 2e-5, desc))
        out.append(('modtail s1', rel(s1, ref_s1), 2e-3 if half else 2e-5, desc))
    return out


# ------------------------------------------------------------------------------------------------
# round5b: the strided native op over dtype x layout x geometry (float64 1e-12, float32 3e-6, fp16 2e-3), the fused modulated
# form on halves (4e-3), the closed double backward of the style factors (2e-4)
# ------------------------------------------------------------------------------------------------

def _case_round5b(seed):
    kk, _, _, orc = _mods()
    from shgan_amd.model_zoo import stylegan as sg
    from shgan_amd.model_zoo.stylegan_utils import upfirdn2d as ufd
    rnd = random.Random(seed)
    torch.manual_seed(seed)
    tol = {torch.float64: 1e-12, torch.float32: 3e-6, torch.float16: 2e-3}
    out = []
    dt = rnd.choice([torch.float64, torch.float32, torch.float16])
    n, c, h, w = rnd.randint(1, 3), rnd.randint(1, 9), rnd.randint(1, 20), rnd.randint(1, 20)
    layout = rnd.choice(['nchw', 'cl', 'view', 'tview'])
    if layout == 'view':
        big = torch.randn(n, c + 2, h + 3, w + 5, dtype=torch.float64).to(dt).to(DEV)
        x = big[:, 1:c + 1, 2:h + 2, 1:w + 1]
    elif layout == 'tview':
        x = torch.randn(n, c, w, h, dtype=torch.float64).to(dt).to(DEV).transpose(2, 3)
    else:
        x = torch.randn(n, c, h, w, dtype=torch.float64).to(dt).to(DEV)
        if layout == 'cl':
            x = x.contiguous(memory_format=CL)
    fh, fw = rnd.randint(1, 6), rnd.randint(1, 6)
    f = torch.randn(fw, fh, device=DEV).t() if rnd.random() < 0.5 else torch.randn(fh, fw, device=DEV)
    upx, upy, dnx, dny = rnd.randint(1, 3), rnd.randint(1, 3), rnd.randint(1, 3), rnd.randint(1, 3)
    pad = [rnd.randint(-2, 5) for _ in range(4)]
    ow = (w * upx + pad[0] + pad[1] - fw + dnx) // dnx
    oh = (h * upy + pad[2] + pad[3] - fh + dny) // dny
    if oh >= 1 and ow >= 1 and h * upy + pad[2] + pad[3] >= fh and w * upx + pad[0] + pad[1] >= fw:
        flip, gain = rnd.random() < 0.5, float(np.float32(rnd.choice([1.0, 4.0, 0.3])))
        y = kk.upfirdn2d_strided(x, f, upx, upy, dnx, dny, pad[0], pad[1], pad[2], pad[3], flip, gain)
        ref = orc.upfirdn2d(x.cpu().double(), f.cpu().contiguous().double(), up=[upx, upy], down=[dnx, dny], padding=pad, flip_filter=flip, gain=gain)
        desc = f'{dt} {layout} {(n, c, h, w)} f{(fh, fw)} up/down{(upx, upy, dnx, dny)} pad{pad}'
        ok = tuple(y.shape) == tuple(ref.shape) and y.dtype == dt
        e = (rel(y, ref) if float(ref.abs().max()) > 0 else 0.0) if ok else 1.0
        out.append(('strided', e, tol[dt], desc))
    n, i, o = rnd.randint(1, 3), 8 * rnd.randint(1, 8), rnd.choice([3, 8, 24, 40, 64])
    k = rnd.choice([1, 3]) if o != 3 else 1
    up = rnd.choice([1, 2]) if (k == 3 and o % 8 == 0) else 1
    demod = o != 3
    if not demod:
        up = 1
    hh, ww = rnd.randint(4, 24), rnd.randint(4, 24)
    xh = (torch.randn(n, i, hh, ww) * 2).half().to(DEV).to(memory_format=CL)
    wt = torch.randn(o, i, k, k, device=DEV)
    st = torch.randn(n, i, device=DEV) + 1.0
    noise = (torch.randn(hh * up, ww * up, device=DEV) * 0.1) if (demod and rnd.random() < 0.6) else None
    f4 = ufd.setup_filter([1, 3, 3, 1]).to(DEV)
    kw = dict(weight=wt, styles=st, noise=noise, up=up, padding=k // 2, resample_filter=f4 if up > 1 else None, demodulate=demod, flip_weight=(up == 1))
    y = sg.modulated_conv2d(x=xh, fused_modconv=True, **kw)
    ref = orc.modulated_conv2d(xh.cpu().double().contiguous(), wt.cpu().double(), st.cpu().double(), noise=None if noise is None else noise.cpu().double(),
                               up=up, padding=k // 2, resample_filter=f4.cpu().double() if up > 1 else None, demodulate=demod, flip_weight=(up == 1))
    out.append(('fused_half', rel(y, ref) if y.dtype == torch.float16 else 1.0, 4e-3, f'n{n} {i}->{o} k{k} up{up} {hh}x{ww} noise{noise is not None}'))
    n, i, o, half = rnd.randint(1, 8), rnd.choice([8, 24, 64, 200, 512]), rnd.choice([3, 16, 64, 300, 512]), rnd.random() < 0.5
    g = torch.Generator().manual_seed(seed * 100003)

    def mk(*sh):
        return torch.randn(*sh, generator=g, dtype=torch.float64).to(DEV)
    s64, w64 = mk(n, i) + 1.0, torch.rand(o, i, generator=g, dtype=torch.float64).to(DEV) * 0.01
    a64, b64, A64, B64 = mk(n, i), mk(n, o), mk(n, i), mk(o, i)

    def ref_fn(s, w_):
        if half:
            s = s / s.norm(float('inf'), dim=1, keepdim=True)
        s = s * s.square().mean().rsqrt()
        return s, (s.square().matmul(w_.t()) + 1e-8).rsqrt()

    def run(fn, dt_):
        s, w_, a, b = (t.to(dt_).clone().requires_grad_(True) for t in (s64, w64, a64, b64))
        with torch.enable_grad():
            sn, d = fn(s, w_)
            gs, gw = torch.autograd.grad([sn, d], [s, w_], [a, b], create_graph=True)
            return torch.autograd.grad((gs * A64.to(dt_)).sum() + (gw * B64.to(dt_)).sum(), [s, w_, a, b])
    if n * i <= 8192:
        want, got = run(ref_fn, torch.float64), run(lambda s, w_: sg._StyleFactorsFn.apply(s, w_, half), torch.float32)
        out.append(('style_bwd', max(rel(u, v) for u, v in zip(got, want)), 2e-4, f'n{n} i{i} o{o} half{half}'))
    return out


# ------------------------------------------------------------------------------------------------
# round6: the unmasked weight gradient and its dispatch boundary, 1x1 weight gradients, the 1x1 GEMM form (3e-5)
# ------------------------------------------------------------------------------------------------

def _case_round6(seed, full=False):
    kk, _, _, _ = _mods()
    rs = np.random.RandomState(seed)
    out = []
    n = int(rs.randint(1, 5 if full else 3)); ci = int(rs.choice([64, 128, 192, 48] if full else [64, 128, 48])); co = int(rs.choice([64, 128, 40]))
    ow = int(rs.choice([4, 8, 16, 32, 64, 96, 24] if full else [4, 8, 16, 32, 64, 24])); oh = int(rs.choice([4, 8, 10, 16, 33] if full else [4, 8, 10, 16]))
    w_ = 2 * ow + int(rs.choice([1, 1, 1, 2])); h_ = 2 * oh + int(rs.choice([1, 2]))
    x = torch.from_numpy(rs.standard_normal((n, ci, h_, w_)).astype(np.float32))
    g = torch.from_numpy(rs.standard_normal((n, co, (h_ - 3) // 2 + 1, (w_ - 3) // 2 + 1)).astype(np.float32))
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 3, 3), g.double(), stride=2, padding=0)
    out.append(('wgrad s2', rel(kk.conv2d_wgrad(x.to(DEV), g.to(DEV), 3, 3, 2, 0), ref), 3e-5, f'n{n} {ci}->{co} {h_}x{w_}'))
    hh, ww = [(8, 8), (16, 32), (4, 16), (24, 24), (64, 64), (5, 13)][rs.randint(6)]
    ci = int(rs.choice([64, 128, 72])); co = int(rs.choice([64, 192, 24]))
    x = torch.from_numpy(rs.standard_normal((n, ci, hh, ww)).astype(np.float32))
    g = torch.from_numpy(rs.standard_normal((n, co, hh, ww)).astype(np.float32))
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 1, 1), g.double())
    out.append(('wgrad 1x1', rel(kk.conv2d_wgrad(x.to(DEV), g.to(DEV), 1, 1, 1, 0), ref), 3e-5, f'n{n} {ci}->{co} {hh}x{ww}'))
    n = int(rs.choice([1, 4, 8, 16] if full else [1, 4, 8])); ci = int(rs.choice([16, 32, 64, 80, 128] if full else [16, 32, 64, 80]))
    co = int(rs.choice([64, 128, 192, 256, 100]))
    sizes = [(16, 16), (32, 32), (64, 32), (128, 128), (24, 24), (64, 64)] if full else [(16, 16), (32, 32), (64, 32), (24, 24), (64, 64)]
    hh, ww = sizes[rs.randint(len(sizes))]
    x = torch.from_numpy(rs.standard_normal((n, ci, hh, ww)).astype(np.float32))
    wt = torch.from_numpy((rs.standard_normal((co, ci, 1, 1)) / np.sqrt(ci)).astype(np.float32))
    bias = torch.from_numpy(rs.standard_normal(co).astype(np.float32)) if rs.rand() < 0.5 else None
    res = torch.from_numpy(rs.standard_normal((n, co, hh, ww)).astype(np.float32)) if rs.rand() < 0.5 else None
    act = bool(rs.rand() < 0.5); gain = float(rs.choice([1.0, 0.5, np.sqrt(0.5)]))
    z = F.conv2d(x.double(), wt.double(), None if bias is None else bias.double())
    if act:
        z = torch.where(z < 0, z * 0.2, z) * (np.sqrt(2.0) * gain)
        z = z.clamp(-256.0 * gain, 256.0 * gain)
    else:
        z = z * gain
    if res is not None:
        z = z + res.double()
    xd = x.to(DEV)
    unaligned = bool(rs.rand() < 0.2)
    if unaligned:                                       # a view that is not 16-byte aligned
        xd = torch.zeros(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(xd)
    got = kk.conv2d(xd, kk.conv_weight_prep(wt.to(DEV)), mode=0, pad=0, bias=None if bias is None else bias.to(DEV), act=act, gain=gain,
                    residual=None if res is None else res.to(DEV))
    out.append(('conv 1x1', rel(got, z), 3e-5, f'n{n} {ci}->{co} {hh}x{ww} act{act} gain{gain:.3f} bias{bias is not None} '
                                               f'res{res is not None} unaligned{unaligned}'))
    return out


# ------------------------------------------------------------------------------------------------
# f16: the fp16 entry points against float64 on the same half-rounded operands (3e-3)
# ------------------------------------------------------------------------------------------------

def _case_f16(seed):
    _, kf, _, orc = _mods()
    rs = np.random.RandomState(seed)

    def Hh(*shape, scale=1.0):
        return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).half()

    def d(t):
        return t.to(DEV).to(memory_format=CL) if t.ndim == 4 else t.to(DEV)

    kind = rs.choice(['conv', 'conv_fused', 'convT', 'wgrad', 'fir', 'tail'])
    n = int(rs.choice([1, 2, 3]))
    ci = int(rs.choice([4, 8, 16, 24, 32, 40, 64, 96, 136]))
    co = int(rs.choice([3, 8, 16, 24, 32, 40, 64, 72, 136]))
    h = int(rs.choice([4, 5, 8, 9, 16, 17, 31, 32, 33, 40]))
    w = int(rs.choice([4, 7, 8, 16, 17, 31, 33, 36, 48, 65]))
    k = int(rs.choice([1, 3])); s = int(rs.choice([1, 2]))
    desc = f'{kind} n{n} ci{ci} co{co} {h}x{w} k{k} s{s}'
    if kind in ('conv', 'conv_fused'):
        pad = int(rs.choice([0, 1])) if k == 3 else 0
        if (h + 2 * pad - k) // s + 1 < 1 or (w + 2 * pad - k) // s + 1 < 1 or (k == 1 and s == 2):
            return []
        x, wt, b = Hh(n, ci, h, w), Hh(co, ci, k, k, scale=1 / np.sqrt(ci * k * k)), torch.from_numpy(rs.standard_normal(co).astype(np.float32))
        ref = F.conv2d(x.double(), wt.double(), None, stride=s, padding=pad)
        if kind == 'conv':
            ref = ref + b.double().view(1, -1, 1, 1)
            y = kf.conv2d(d(x), wt.to(DEV), b.to(DEV), s, pad)
        else:
            si = torch.from_numpy((rs.rand(n, ci) + 0.5).astype(np.float32)); so = torch.from_numpy((rs.rand(n, co) + 0.5).astype(np.float32))
            nz = torch.from_numpy(rs.standard_normal((n, 1, ref.shape[2], ref.shape[3])).astype(np.float32))
            res = Hh(*ref.shape)
            xs = (x.float() * si.half().float().view(n, ci, 1, 1)).half()
            ref = F.conv2d(xs.double(), wt.double(), None, stride=s, padding=pad).half().double()
            ref = (F.leaky_relu(ref * so.double().view(n, co, 1, 1) + nz.double() * 0.5 + b.double().view(1, -1, 1, 1), 0.2) * np.sqrt(2)).clamp(-256, 256)
            ref = ref.half().double() + res.double()
            y = kf.conv2d(d(x), wt.to(DEV), b.to(DEV), s, pad, in_scale=si.to(DEV), out_scale=so.to(DEV), noise=nz.to(DEV), noise_strength=0.5, act=True,
                          residual=d(res))
        e = rel(y, ref)
    elif kind == 'convT':
        pad = int(rs.choice([0, 1]))
        x, wt = Hh(n, ci, h, w), Hh(ci, co, 3, 3, scale=1 / np.sqrt(ci * 9))
        full = F.conv_transpose2d(x.double(), wt.double(), stride=2)
        oh, ow = int(rs.choice([2 * h + 1 - 2 * pad, 2 * h + 2 - pad, 2 * h - 1])), int(rs.choice([2 * w + 1 - 2 * pad, 2 * w + 2 - pad, 2 * w - 1]))
        ref = torch.zeros(n, co, oh, ow, dtype=torch.float64)
        hh, ww = min(oh, full.shape[2] - pad), min(ow, full.shape[3] - pad)
        ref[:, :, :hh, :ww] = full[:, :, pad:pad + hh, pad:pad + ww]
        desc += f' pad{pad} out{(oh, ow)}'
        e = rel(kf.conv_transpose2d(d(x), wt.to(DEV), None, pad, (oh, ow)), ref)
    elif kind == 'wgrad':
        pad = int(rs.choice([0, 1])) if k == 3 else 0
        if (k == 1 and s == 2) or (h + 2 * pad - k) // s + 1 < 1 or (w + 2 * pad - k) // s + 1 < 1:
            return []
        x = Hh(n, ci, h, w)
        g = Hh(n, co, (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1)
        ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), g.double(), stride=s, padding=pad)
        desc += f' pad{pad}'
        e = rel(kf.conv2d_wgrad(d(x), d(g), k, s, pad), ref)
    elif kind == 'fir':
        c8 = int(rs.choice([8, 16, 24, 64]))
        x = Hh(n, c8, h, w)
        f = torch.from_numpy(rs.rand(int(rs.choice([1, 3, 4])), int(rs.choice([2, 4]))).astype(np.float32))
        pad = [int(v) for v in rs.randint(0, 4, 4)]
        up, down = int(rs.choice([1, 1, 2])), int(rs.choice([1, 1, 2]))
        flip, gain = bool(rs.randint(2)), float(rs.choice([1.0, 4.0, 0.37]))
        try:
            ref = orc.upfirdn2d(x.double(), f.double(), up=up, down=down, padding=pad, flip_filter=flip, gain=gain)
        except Exception:
            return []
        if ref.shape[2] < 1 or ref.shape[3] < 1:
            return []
        desc = f'fir n{n} c{c8} {h}x{w} f{tuple(f.shape)} up{up} down{down} pad{pad} flip{flip} gain{gain}'
        e = rel(kf.upfirdn2d(d(x), f.to(DEV), up, up, down, down, pad[0], pad[1], pad[2], pad[3], flip, gain), ref)
    else:
        c8 = int(rs.choice([8, 16, 32, 64, 128, 512]))
        hw = (int(rs.choice([3, 8, 12])), int(rs.choice([5, 16, 20])))
        t, dd, b = Hh(n, c8, *hw, scale=30), torch.from_numpy((rs.rand(n, c8) + 0.5).astype(np.float32)), torch.from_numpy(rs.standard_normal(c8).astype(np.float32))
        nz = torch.from_numpy(rs.standard_normal((n, 1) + hw).astype(np.float32))
        gy = Hh(n, c8, *hw)
        with torch.enable_grad():
            tr, dr = t.double().requires_grad_(True), dd.double().requires_grad_(True)
            yr = (F.leaky_relu(tr * dr.view(n, c8, 1, 1) + nz.double() + b.double().view(1, -1, 1, 1), 0.2) * np.sqrt(2)).clamp(-256, 256)
            yr.backward(gy.double())
        y = kf.modtail(d(t), dd.to(DEV), nz.to(DEV), b.to(DEV), act=True)
        gt, s1, _, _ = kf.modtail_backward(d(gy), y, d(t), dd.to(DEV), want_sums=True, want_noise=True, act=True)
        bad = (gt.float().cpu() - tr.grad.float()).abs() > 3e-3 * tr.grad.abs().max()       # (clamp sliver, tests/test_gpu_fp16.py)
        desc = f'tail n{n} c{c8} {hw}'
        e = max(rel(y, yr), rel(s1, dr.grad), 0.0 if bad.float().mean() < 3e-3 else 1.0)
    return [(kind, e, 3e-3, desc)]


# family -> (case function, first seed, number of cases) of the suite
FAMILIES = {
    'ops': (_case_ops, 1000, 32),
    'fir_march': (_case_fir_march, 2000, 32),
    'round4': (_case_round4, 4000, 16),
    'round5': (_case_round5, 5000, 16),
    'round5b': (_case_round5b, 5500, 24),
    'round6': (_case_round6, 6000, 16),
    'f16': (_case_f16, 7000, 32),
}
FULL = ('ops', 'round5', 'round6')          # the families that take full=True
