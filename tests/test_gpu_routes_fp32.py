"""Route table of the float32 entry points of shgan_amd.kernels (run with -m gpu on an MI355X).

Every entry point picks one of several HIP kernels -- often one of several template instantiations -- from the shape, the alignment of its
pointers, its epilogue arguments and the module switches.  Each case below names the kernel (or instantiation) that must serve its input and
the ones that must not, and compares the result with a float64 CPU evaluation of the same math.  The cases sit one step either side of every
dispatch predicate, so a changed constant or predicate moves a case off its route and fails it.  The last test checks that the table covers
every kernel these entry points can launch (the hipLaunchKernelGGL sites of the .hip sources).

What happens INSIDE a route -- the tail split of the one-workgroup-per-CU direct kernels, ragged and halved K splits and their grid-stride
reductions, tile_search's tile shapes, second trips of the plane-walking FIR kernels, partial workgroups of the marching kernels, several chunks
per weight-gradient slice -- is held to float64 in test_gpu_loop_bounds_fp32.py (the launch plans on the host in plan_f32.py and
test_plan_f32_cpu.py); the cases here are a few workgroups each and reach none of it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from route_probe import any_hit, launched

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SQRT2 = 2 ** 0.5
TOL_CONV = 2e-5          # convolutions and their weight gradients (tests/test_gpu_wgrad_wino.py, the ops family of tests/fuzz_cases.py)
TOL_PW = 1e-5            # elementwise / FIR passes


def _kk():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels
    return kernels


def _orc():
    from oracle import shgan_oracle as orc
    return orc


def rnd(seed, *shape, scale=1.0, lo=None):
    rs = np.random.RandomState(seed)
    a = rs.rand(*shape) + lo if lo is not None else rs.standard_normal(shape) * scale
    return torch.from_numpy(a.astype(np.float32))


def dev(t, offset=0):
    """t on the GPU; ``offset`` (floats): as a contiguous view that far into a fresh allocation (1: data_ptr() % 16 == 4; 4: 16-byte aligned
    but not 32-byte aligned)."""
    if t is None:
        return None
    if not offset:
        return t.to(DEV)
    offset = int(offset)
    buf = torch.zeros(t.numel() + offset, device=DEV)
    v = buf[offset:].view(t.shape).copy_(t.to(DEV))
    assert v.is_contiguous() and buf.data_ptr() % 256 == 0 and v.data_ptr() % 64 == 4 * offset
    return v


def act64(z, act, gain=1.0, alpha=0.2, act_gain=SQRT2, clamp=256.0):
    if not act:
        return z * gain
    z = torch.where(z < 0, z * alpha, z) * (act_gain * gain)
    return z.clamp(-clamp * gain, clamp * gain) if clamp is not None else z


# ------------------------------------------------------------------------------------------------
# case builders: each returns (call, ref, tol); ``call()`` runs on the GPU and returns a tensor (or a list of tensors), ``ref`` the float64
# counterpart(s); the inputs are built before the probe, so only the entry point's own launches are traced
# ------------------------------------------------------------------------------------------------

def conv_same(nb, i, o, h, w, k=3, offset=False, bias=True, act=True, residual=None):
    """3x3 'same' (or 1x1) convolution + bias + activation (+ ``residual``: None | 'aligned' | 'offset')."""
    kk = _kk()
    x, wt = rnd(1, nb, i, h, w), rnd(2, o, i, k, k)
    g = 1.0 / np.sqrt(i * k * k)
    b = rnd(3, o) if bias else None
    res = rnd(4, nb, o, h, w) if residual else None
    z = F.conv2d(x.double(), wt.double() * g, padding=k // 2)
    if b is not None:
        z = z + b.double().view(1, -1, 1, 1)
    ref = act64(z, act, gain=0.7)
    if res is not None:
        ref = ref + res.double()
    xd, pw = dev(x, offset), kk.conv_weight_prep(wt.to(DEV), gain=g)
    bd, rd = dev(b), dev(res, residual == 'offset')
    return (lambda: kk.conv2d(xd, pw, mode=kk.MODE_SAME, pad=k // 2, bias=bd, act=act, gain=0.7, residual=rd)), ref, TOL_CONV


def conv_down(nb, i, o, h, w, in_scale=False):
    kk = _kk()
    x, wt, b = rnd(5, nb, i, h, w), rnd(6, o, i, 3, 3), rnd(7, o)
    s = rnd(8, nb, i, lo=0.5) if in_scale else None
    g = 1.0 / np.sqrt(i * 9)
    xs = x.double() * (s.double()[:, :, None, None] if in_scale else 1.0)
    ref = act64(F.conv2d(xs, wt.double() * g, stride=2) + b.double().view(1, -1, 1, 1), True)
    xd, pw, bd, sd = dev(x), kk.conv_weight_prep(wt.to(DEV), gain=g), dev(b), dev(s)
    return (lambda: kk.conv2d(xd, pw, mode=kk.MODE_DOWN2, pad=0, in_scale=sd, bias=bd, act=True)), ref, TOL_CONV


def conv_up(nb, i, o, h, w, planar=True, bias=False, offset=False):
    """Stride-2 transposed 3x3 convolution; planar output = the four phase planes [4, NB, O, H+1, W+1] (valid extent compared)."""
    kk = _kk()
    x, wt = rnd(9, nb, i, h, w), rnd(10, o, i, 3, 3)
    b = rnd(11, o) if bias else None
    g = 1.0 / np.sqrt(i * 9)
    full = F.conv_transpose2d(x.double(), (wt.double() * g).transpose(0, 1), stride=2)
    if b is not None:
        full = full + b.double().view(1, -1, 1, 1)
    xd, pw, bd = dev(x, offset), kk.conv_weight_prep(wt.to(DEV), gain=g), dev(b)

    def call():
        y = kk.conv2d(xd, pw, mode=kk.MODE_UP2T, bias=bd, planar=planar)
        if not planar:
            return y
        return torch.cat([y[a * 2 + c][:, :, :h + 1 - a, :w + 1 - c].reshape(-1) for a in range(2) for c in range(2)])
    if planar:
        full = torch.cat([full[:, :, a::2, c::2].reshape(-1) for a in range(2) for c in range(2)])
    return call, full, TOL_CONV


def down_layer(i, o, h, w):
    """The FIR-filtered stride-2 3x3 layer through its own forward (stylegan.conv2d_layer, down=2)."""
    kk = _kk()
    from shgan_amd.model_zoo import stylegan
    torch.manual_seed(12)
    layer = stylegan.conv2d_layer(i, o, 3, activation='lrelu_agc(alpha=0.2, gain=sqrt_2, clamp=256)', down=2)
    layer.bias.data.copy_(rnd(13, o))
    x = rnd(14, 1, i, h, w)
    f = layer.resample_filter.double()
    xf = _orc().upfirdn2d(x.double(), f, padding=[2, 2, 2, 2])
    ref = act64(F.conv2d(xf, layer.weight.detach().double() * layer.weight_gain, stride=2) + layer.bias.detach().double().view(1, -1, 1, 1), True)
    layer = layer.to(DEV)
    xd = dev(x)
    return (lambda: layer(xd)), ref, TOL_CONV


def fir_conv_down2(nb, i, o, h, w, offset=False, sep=True):
    kk = _kk()
    orc = _orc()
    x, wt, b = rnd(15, nb, i, h, w), rnd(16, o, i, 3, 3), rnd(17, o)
    f = orc.setup_filter([1, 3, 3, 1]) if sep else rnd(18, 4, 4, lo=0.1)
    g = 1.0 / np.sqrt(i * 9)
    xf = orc.upfirdn2d(x.double(), f.double(), padding=[2, 2, 2, 2])
    ref = act64(F.conv2d(xf, wt.double() * g, stride=2) + b.double().view(1, -1, 1, 1), True)
    xd, fd, pw, bd = dev(x, offset), dev(f), kk.conv_weight_prep(wt.to(DEV), gain=g), dev(b)
    assert kk.down_poly_supported(xd, pw, force=True)
    return (lambda: kk.fir_conv_down2(xd, fd, pw, bias=bd, act=True)), ref, TOL_CONV


def thin_in(i, o, h, w):
    kk = _kk()
    x, wt, b = rnd(19, 2, i, h, w), rnd(20, o, i), rnd(21, o)
    g = 1.0 / np.sqrt(i)
    ref = act64(torch.einsum('nihw,oi->nohw', x.double(), wt.double() * g) + b.double().view(1, -1, 1, 1), True)
    xd, wd, bd = dev(x), dev(wt), dev(b)
    return (lambda: kk.conv1x1_thin_in(xd, wd, bd, wgain=g, act=True)), ref, TOL_CONV


def wgrad(nb, i, o, h, w, k=3, stride=1, pad=1, offset=False):
    kk = _kk()
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x, g = rnd(22, nb, i, h, w), rnd(23, nb, o, oh, ow)
    ref = torch.nn.grad.conv2d_weight(x.double(), (o, i, k, k), g.double(), stride=stride, padding=pad)
    xd, gd = dev(x, offset), dev(g)
    return (lambda: kk.conv2d_wgrad(xd, gd, k, k, stride, pad)), ref, TOL_CONV


def fir(n, c, h, w, up=1, down=1, pad=(2, 2, 2, 2), sep=True, offset=False, flip=False, gain=1.0):
    kk = _kk()
    orc = _orc()
    x = rnd(24, n, c, h, w)
    f = orc.setup_filter([1, 3, 3, 1]) if sep else rnd(25, 4, 4, lo=0.1)
    ref = orc.upfirdn2d(x.double(), f.double(), up=up, down=down, padding=list(pad), flip_filter=flip, gain=gain)
    xd, fd = dev(x, offset), dev(f)
    return (lambda: kk.upfirdn2d(xd, fd, upx=up, upy=up, downx=down, downy=down, padx0=pad[0], padx1=pad[1], pady0=pad[2], pady1=pad[3],
                                 flip=flip, gain=gain)), ref, TOL_PW


def fir_strided(dtype, n=2, c=3, h=9, w=11):
    kk = _kk()
    x64 = rnd(26, n, c, w, h).double()
    f = rnd(27, 3, 5)
    xin = x64.to(dtype)
    ref = _orc().upfirdn2d(xin.double().transpose(2, 3), f.double(), up=2, down=1, padding=[1, 2, 0, 1], gain=4.0)
    xd, fd = xin.to(DEV).transpose(2, 3), dev(f)                     # H and W strides exchanged: read in place
    tol = {torch.float64: 1e-12, torch.float32: 3e-6, torch.float16: 2e-3}[dtype]       # (the round5b family of tests/fuzz_cases.py)
    return (lambda: kk.upfirdn2d_strided(xd, fd, 2, 2, 1, 1, 1, 2, 0, 1, False, 4.0)), ref, tol


def upfir_planar(n, c, h, w, sep=True, res_offset=False, epi=True):
    kk = _kk()
    orc = _orc()
    mid = rnd(28, 4, n, c, h + 1, w + 1)
    f = orc.setup_filter([1, 3, 3, 1]) if sep else rnd(29, 4, 4, lo=0.1)
    full = torch.zeros(n, c, 2 * h + 1, 2 * w + 1, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            full[:, :, a::2, b::2] = mid[a * 2 + b][:, :, :h + 1 - a, :w + 1 - b].double()
    ref = orc.upfirdn2d(full, f.double(), padding=[1, 1, 1, 1], gain=4.0)
    kw = {}
    if epi:
        sc, bi, nz, res = rnd(30, n * c, lo=0.5), rnd(31, c), rnd(32, 1, 1, 2 * h, 2 * w), rnd(33, n, c, 2 * h, 2 * w)
        ref = act64(ref * sc.double().view(n, c, 1, 1) + nz.double() * 0.3 + bi.double().view(1, c, 1, 1), True, gain=0.8) + res.double()
        kw = dict(scale=dev(sc), bias=dev(bi), noise=dev(nz), residual=dev(res, res_offset), noise_strength=0.3, act=True, gain=0.8)
    md, fd = dev(mid), dev(f)
    return (lambda: kk.upfir_planar(md, fd, **kw)), ref, TOL_PW


def bias_act(n=2, c=8, h=16, w=16, x_off=0, noise=None, noise_off=False, res=False, res_off=False, scale=True, bias=True, act=True):
    kk = _kk()
    x = rnd(34, n, c, h, w, scale=3.0)
    sc, bi = (rnd(35, n * c, lo=0.5) if scale else None), (rnd(36, c) if bias else None)
    nz = None if noise is None else rnd(37, (n if noise == 'per' else 1), 1, h, w)
    r = rnd(38, n, c, h, w) if res else None
    z = x.double()
    if sc is not None:
        z = z * sc.double().view(n, c, 1, 1)
    if nz is not None:
        z = z + nz.double() * 0.3
    if bi is not None:
        z = z + bi.double().view(1, c, 1, 1)
    ref = act64(z, act, gain=0.6, clamp=2.0)
    if r is not None:
        ref = ref + r.double()
    xd, nd, rd, sd, bd = dev(x, x_off), dev(nz, noise_off), dev(r, res_off), dev(sc), dev(bi)
    return (lambda: kk.bias_act(xd, bias=bd, scale=sd, noise=nd, noise_strength=0.3, residual=rd, act=act, gain=0.6, clamp=2.0)), ref, TOL_PW


def _on_clamp_values(n, clamp):
    """Values on the clamp and one float32 ulp either side of it, both signs, among ordinary ones."""
    c32 = np.float32(clamp)
    edge = np.array([c32, np.nextafter(c32, np.float32(0)), np.nextafter(c32, np.float32(np.inf))], np.float32)
    v = np.random.RandomState(39).standard_normal(n).astype(np.float32) * clamp
    v[:6] = np.concatenate([edge, -edge])
    return torch.from_numpy(v)


def bias_act_clamp(hw):
    """Forward inputs whose activation lands exactly on +-clamp (act_gain 1: lrelu(x) * 1 = x; the negative side x / alpha)."""
    kk = _kk()
    clamp, alpha = 4.0, 0.25
    v = _on_clamp_values(2 * 4 * hw, clamp)
    v[6:12] = torch.tensor([4.0, -16.0, 3.0, -12.0, 4.5, -17.0])
    x = v.view(2, 4, 1, hw)
    ref = act64(x.double(), True, alpha=alpha, act_gain=1.0, clamp=clamp)
    xd = dev(x)
    return (lambda: kk.bias_act(xd, act=True, alpha=alpha, act_gain=1.0, clamp=clamp)), ref, 0.0


def bias_act_bwd(act):
    """dL/dx from the forward OUTPUT y: zero slope at |y| >= clamp (y exactly on the clamp included), the full slope one ulp inside."""
    kk = _kk()
    clamp = 4.0
    y = _on_clamp_values(4096, clamp).view(2, 8, 16, 16)
    g = rnd(40, 2, 8, 16, 16)
    yd = y.double()
    if act:
        slope = torch.where(yd.abs() >= clamp, torch.zeros_like(yd), torch.where(yd > 0, torch.full_like(yd, SQRT2), torch.full_like(yd, 0.2 * SQRT2)))
    else:
        slope = torch.full_like(yd, 0.5)
    ref = g.double() * slope
    gd, ydv = dev(g), dev(y)
    kw = dict(act=True, clamp=clamp) if act else dict(act=False, gain=0.5)
    return (lambda: kk.bias_act_backward(gd, ydv, **kw)), ref, TOL_PW


def torgb(n, i, o, h, w, base=False):
    kk = _kk()
    orc = _orc()
    x, wt, st, b = rnd(41, n, i, h, w), rnd(42, o, i), rnd(43, n, i, lo=0.5), rnd(44, o)
    ref = torch.einsum('nihw,oi,ni->nohw', x.double(), wt.double(), st.double()) + b.double().view(1, -1, 1, 1)
    bu = f = None
    if base:
        bu, f = rnd(45, n, o, h // 2, w // 2), orc.setup_filter([1, 3, 3, 1])
        ref = ref + orc.upsample2d(bu.double(), f.double())
    xd, wd, sd, bd, bud, fd = dev(x), dev(wt), dev(st), dev(b), dev(bu), dev(f)
    return (lambda: kk.torgb(xd, wd, sd, bd, base_up=bud, f=fd)), ref, TOL_PW


def mbstd(n, c, h, w, group, f=1):
    kk = _kk()
    x = rnd(46, n, c, h, w)
    g = n if group is None else min(group, n)
    y = x.double().reshape(g, -1, f, c // f, h, w)
    y = (y - y.mean(dim=0)).square().mean(dim=0)
    y = (y + 1e-8).sqrt().mean(dim=[2, 3, 4]).reshape(-1, f, 1, 1).repeat(g, 1, h, w)
    ref = torch.cat([x.double(), y], dim=1)
    xd = dev(x)
    return (lambda: kk.minibatch_std(xd, group, f)), ref, TOL_PW


# ------------------------------------------------------------------------------------------------
# the table: id -> (builder, expect, forbid, switches)
# ------------------------------------------------------------------------------------------------
MFMA = 'conv_mfma_kernel'
S1_DB, S1_NARROW, S1_WIDE = (f'{MFMA}<9, 8, 2, 2, 2, 4, 1, false, true, 2>', f'{MFMA}<9, 8, 2, 2, 1, 4, 2, false, false, 3>',
                             f'{MFMA}<9, 8, 2, 2, 2, 2, 2, false, false, 2>')
S2_DB, S2_NARROW, S2_WIDE = (f'{MFMA}<9, 8, 1, 2, 4, 4, 2, false, true, 4>', f'{MFMA}<9, 8, 2, 2, 1, 4, 5, false, false, 2>',
                             f'{MFMA}<9, 8, 2, 2, 2, 2, 3, false, false, 2>')
UP_RAW_N, UP_RAW_W = f'{MFMA}<9, 8, 1, 1, 2, 8, 1, true, true, 4>', f'{MFMA}<9, 8, 1, 1, 4, 4, 1, true, true, 4>'
UP_EPI_N, UP_EPI_W, UP_SMALL = (f'{MFMA}<9, 8, 2, 1, 1, 8, 1, true, true, 2>', f'{MFMA}<9, 8, 2, 1, 2, 4, 1, true, true, 2>',
                                f'{MFMA}<9, 8, 2, 1, 1, 4, 2, true, false, 2>')
C1_N, C1_W = f'{MFMA}<1, 32, 2, 2, 1, 4, 1, false, false, 3>', f'{MFMA}<1, 32, 2, 2, 2, 2, 1, false, false, 3>'
WINO, WINO4, POLY_UP, POLY_DOWN = 'conv_wino_kernel', 'conv_wino4_kernel', 'conv_poly_up_kernel', 'conv_poly_down_kernel'
WSPLIT, MSPLIT, WGW = 'wino_split_reduce_kernel', 'splitk_reduce_kernel', 'wgw::conv_wgrad_wino_kernel'
FDM = 'fir_down_march_kernel'


def C(builder, expect, forbid=(), switches=None):
    return (builder, tuple(expect), tuple(forbid), dict(switches or {}))


CASES = {
    # ---- conv2d, same mode: F(2x2) from WINO_MIN rows, F(4x4) from WINO4_MIN, direct kernel otherwise
    'same_h_eq_wino_min': C(lambda: conv_same(1, 16, 32, 16, 16), [f'{WINO}<8, 8>'], [MFMA, WINO4, WSPLIT]),
    'same_h_below_wino_min': C(lambda: conv_same(1, 16, 32, 15, 16), [S1_NARROW], [WINO, WINO4, MSPLIT]),
    'same_h_eq_wino4_min': C(lambda: conv_same(1, 16, 32, 32, 32), [f'{WINO4}<4, 8>'], [MFMA, WINO]),
    'same_h_below_wino4_min': C(lambda: conv_same(1, 16, 32, 31, 32), [f'{WINO}<4, 16>'], [MFMA, WINO4]),
    'same_w_mod4_0': C(lambda: conv_same(1, 16, 32, 16, 20), [f'{WINO}<8, 8>'], [MFMA, WINO4]),
    'same_w_mod4_2': C(lambda: conv_same(1, 16, 32, 16, 18), [S1_NARROW], [WINO, WINO4]),
    'same_x_unaligned': C(lambda: conv_same(1, 16, 32, 16, 16, offset=True), [S1_NARROW], [WINO, WINO4]),
    'same_x_unaligned_db': C(lambda: conv_same(1, 16, 128, 32, 32, offset=True), [S1_DB], [WINO, WINO4]),
    'same_i_1024': C(lambda: conv_same(1, 1024, 64, 16, 16), [f'{WINO}<8, 8>', WSPLIT], [MFMA, WINO4]),
    'same_i_1025': C(lambda: conv_same(1, 1025, 64, 16, 16), [S1_NARROW, MSPLIT], [WINO, WINO4]),
    'same_wino4_unsupported_w16': C(lambda: conv_same(1, 16, 32, 32, 16), [f'{WINO}<8, 8>'], [MFMA, WINO4]),
    'same_wino4_8x64_tiles': C(lambda: conv_same(1, 8, 16, 32, 128), [f'{WINO4}<2, 16>'], [MFMA, WINO]),
    'same_wino4_4x128_tiles': C(lambda: conv_same(1, 8, 16, 32, 256), [f'{WINO4}<1, 32>'], [MFMA, WINO]),
    'same_wino4_split': C(lambda: conv_same(1, 256, 64, 32, 32), [f'{WINO4}<4, 8>', WSPLIT], [MFMA, WINO]),
    'same_wino4_split_off': C(lambda: conv_same(1, 256, 64, 32, 32), [f'{WINO4}<4, 8>'], [MFMA, WINO, WSPLIT], {'WINO_SPLIT': False}),
    'same_wino_split_off': C(lambda: conv_same(1, 1024, 64, 16, 16), [f'{WINO}<8, 8>'], [MFMA, WSPLIT], {'WINO_SPLIT': False}),
    'same_wino4_off': C(lambda: conv_same(1, 16, 32, 32, 32), [f'{WINO}<4, 16>'], [MFMA, WINO4], {'WINO4': False}),
    'same_wino_off_db': C(lambda: conv_same(1, 16, 128, 32, 32), [S1_DB], [WINO, WINO4], {'WINO': False}),
    'same_wino_off_narrow': C(lambda: conv_same(1, 16, 32, 16, 16), [S1_NARROW], [WINO, WINO4], {'WINO': False}),
    'same_mfma_wide_small': C(lambda: conv_same(1, 16, 128, 15, 16), [S1_WIDE], [WINO, WINO4, MSPLIT]),
    'same_mfma_splitk': C(lambda: conv_same(1, 256, 32, 15, 16), [S1_NARROW, MSPLIT], [WINO, WINO4]),
    # (the F(4x4) kernel wants y / noise / residual 16-byte aligned too: an unaligned residual takes F(2x2), which needs 8 bytes)
    'same_wino4_residual_unaligned': C(lambda: conv_same(1, 16, 32, 32, 32, residual='offset'), [S1_NARROW], [WINO4, WINO]),
    'same_wino4_residual_aligned': C(lambda: conv_same(1, 16, 32, 32, 32, residual='aligned'), [f'{WINO4}<4, 8>'], [MFMA]),
    # ---- 1x1 layers: GEMM form when whole tiles fill the chip and the operands are 16-byte aligned, the tap-list kernel otherwise
    'c1x1_gemm_narrow': C(lambda: conv_same(32, 16, 64, 64, 64, k=1), ['conv1x1_gemm_kernel<1, 4, 16>'], [MFMA]),
    'c1x1_gemm_wide': C(lambda: conv_same(16, 16, 128, 64, 64, k=1), ['conv1x1_gemm_kernel<2, 2, 16>'], [MFMA]),
    'c1x1_taps_unaligned': C(lambda: conv_same(32, 16, 64, 64, 64, k=1, offset=True), [C1_N], ['conv1x1_gemm_kernel']),
    'c1x1_taps_narrow_small': C(lambda: conv_same(1, 16, 64, 16, 16, k=1), [C1_N], ['conv1x1_gemm_kernel']),
    'c1x1_taps_wide_small': C(lambda: conv_same(1, 16, 128, 16, 16, k=1), [C1_W], ['conv1x1_gemm_kernel']),
    'c1x1_thin_in_i3': C(lambda: thin_in(3, 32, 16, 16), ['conv1x1_small_i_kernel<8>'], [MFMA, 'conv1x1_gemm_kernel']),
    # ---- conv2d, stride-2 mode (the direct kernel)
    'down_mfma_db': C(lambda: conv_down(1, 16, 128, 17, 65), [S2_DB], [S2_WIDE]),
    'down_mfma_db_in_scale': C(lambda: conv_down(1, 16, 128, 17, 65, in_scale=True), [S2_WIDE], [S2_DB]),
    'down_mfma_narrow': C(lambda: conv_down(1, 16, 64, 17, 17), [S2_NARROW], [S2_DB]),
    'down_mfma_wide_small': C(lambda: conv_down(1, 16, 128, 17, 17), [S2_WIDE], [S2_DB]),
    # ---- conv2d, transposed mode: polyphase Winograd for the planar output without a tail, the direct kernel otherwise
    'up_poly_8x8_w16': C(lambda: conv_up(1, 16, 32, 16, 16), [f'{POLY_UP}<8, 8, 0, 8, 8>'], [MFMA]),
    'up_poly_flat11': C(lambda: conv_up(1, 16, 32, 16, 32), [f'{POLY_UP}<1, 64, 11, 4, 16>'], [MFMA]),
    'up_poly_flat22': C(lambda: conv_up(1, 16, 32, 16, 64), [f'{POLY_UP}<1, 64, 22, 4, 16>'], [MFMA]),
    'up_poly_flat43': C(lambda: conv_up(1, 16, 32, 16, 128), [f'{POLY_UP}<1, 64, 43, 4, 16>'], [MFMA]),
    'up_poly_wide': C(lambda: conv_up(1, 16, 32, 34, 44), [f'{POLY_UP}<4, 16, 0, 4, 16>'], [MFMA]),
    'up_poly_8x8_wide_b': C(lambda: conv_up(1, 16, 32, 16, 48), [f'{POLY_UP}<8, 8, 0, 4, 16>'], [MFMA]),
    'up_poly_split': C(lambda: conv_up(1, 256, 64, 16, 16), [f'{POLY_UP}<8, 8, 0, 8, 8>', WSPLIT], [MFMA]),
    'up_poly_off': C(lambda: conv_up(1, 16, 32, 16, 32), [UP_RAW_N], [POLY_UP], {'UP_POLY': False}),
    'up_bias_epilogue': C(lambda: conv_up(1, 16, 32, 16, 32, bias=True), [UP_EPI_N], [POLY_UP]),
    'up_x_unaligned': C(lambda: conv_up(1, 16, 32, 16, 32, offset=True), [UP_RAW_N], [POLY_UP]),
    'up_unsupported_w18': C(lambda: conv_up(1, 16, 32, 16, 18), [UP_RAW_N], [POLY_UP]),
    'up_raw_wide': C(lambda: conv_up(1, 16, 128, 16, 32, offset=True), [UP_RAW_W], [POLY_UP]),
    'up_epi_wide': C(lambda: conv_up(1, 16, 128, 16, 32, bias=True), [UP_EPI_W], [POLY_UP]),
    'up_small': C(lambda: conv_up(1, 16, 32, 8, 8), [UP_SMALL], [POLY_UP]),
    'up_full_image': C(lambda: conv_up(1, 16, 32, 16, 16, planar=False), [UP_EPI_N], [POLY_UP]),
    # ---- the FIR-filtered stride-2 layer: polyphase form from DOWN_POLY_MIN_I channels and DOWN_POLY_MIN_OUT output pixels per side
    'downlayer_i_eq_min': C(lambda: down_layer(128, 64, 64, 64), [f'{POLY_DOWN}<2, 1, 64, 11>', f'{POLY_DOWN}<3, 4, 16, 0>', f'{FDM}<1, 8, 0>'], [MFMA]),
    'downlayer_i_below_min': C(lambda: down_layer(127, 64, 64, 64), [S2_NARROW], [POLY_DOWN]),
    'downlayer_out_below_min': C(lambda: down_layer(128, 64, 62, 62), [S2_NARROW], [POLY_DOWN]),
    'downlayer_poly_off': C(lambda: down_layer(128, 64, 64, 64), [S2_NARROW], [POLY_DOWN], {'DOWN_POLY': False}),
    'fir_conv_down2_forced_8x8': C(lambda: fir_conv_down2(1, 16, 32, 32, 32), [f'{POLY_DOWN}<2, 8, 8, 0>', f'{POLY_DOWN}<3, 8, 8, 0>', f'{FDM}<1, 8, 0>'], [MFMA]),
    'fir_conv_down2_flat22': C(lambda: fir_conv_down2(1, 8, 16, 32, 128), [f'{POLY_DOWN}<2, 1, 64, 22>', f'{POLY_DOWN}<3, 2, 32, 0>', f'{FDM}<2, 8, 0>'], [MFMA]),
    'fir_conv_down2_flat43': C(lambda: fir_conv_down2(1, 8, 16, 32, 256), [f'{POLY_DOWN}<2, 1, 64, 43>', 'fir_down_march4_kernel<1, 8, 0>'], [MFMA, FDM]),
    'fir_conv_down2_w512': C(lambda: fir_conv_down2(1, 8, 8, 32, 512), ['fir_down_march4_kernel<2, 8, 0>'], [MFMA, FDM]),
    'fir_conv_down2_w256_unaligned': C(lambda: fir_conv_down2(1, 8, 16, 32, 256, offset=True), [f'{FDM}<4, 8, 0>'], [MFMA, 'fir_down_march4_kernel']),
    'fir_conv_down2_wide_da': C(lambda: fir_conv_down2(1, 8, 16, 68, 96), [f'{POLY_DOWN}<2, 4, 16, 0>', f'{POLY_DOWN}<3, 4, 16, 0>', 'fir_same_kernel'],
                                [MFMA, FDM]),
    'fir_conv_down2_nonsep': C(lambda: fir_conv_down2(1, 16, 32, 32, 32, sep=False), [f'{POLY_DOWN}<2, 8, 8, 0>', 'fir_same_kernel'], [FDM]),
    # ---- weight gradient
    'wgrad_wino_w32': C(lambda: wgrad(2, 16, 16, 8, 32), [f'{WGW}<3>'], ['conv_wgrad_kernel', 'conv_wgrad_packed_kernel', 'conv_wgrad_full_kernel']),
    'wgrad_wino_w16': C(lambda: wgrad(2, 16, 16, 8, 16), [f'{WGW}<2>'], ['conv_wgrad_packed_kernel']),
    'wgrad_wino_w8': C(lambda: wgrad(2, 16, 16, 8, 8), [f'{WGW}<1>'], ['conv_wgrad_packed_kernel']),
    'wgrad_wino_w4': C(lambda: wgrad(2, 16, 16, 8, 4), [f'{WGW}<0>'], ['conv_wgrad_packed_kernel']),
    'wgrad_wino_off_packed_s1': C(lambda: wgrad(2, 16, 16, 8, 16), ['conv_wgrad_packed_kernel<3, 3, 1>'], [WGW], {'WGRAD_WINO': False}),
    'wgrad_wino_x_unaligned': C(lambda: wgrad(2, 16, 16, 6, 20, offset=True), ['conv_wgrad_kernel<3, 3, 1, 1>'], [WGW, 'conv_wgrad_packed_kernel']),
    'wgrad_wino_w_mod4_2': C(lambda: wgrad(2, 16, 16, 6, 18), ['conv_wgrad_kernel<3, 3, 1, 1>'], [WGW]),
    'wgrad_two_rows': C(lambda: wgrad(1, 16, 16, 10, 34, pad=0), ['conv_wgrad_kernel<3, 3, 1, 2>'], [WGW]),
    'wgrad_packed_s2': C(lambda: wgrad(1, 16, 16, 17, 17, stride=2, pad=0), ['conv_wgrad_packed_kernel<3, 3, 2>'], ['conv_wgrad_full_kernel']),
    'wgrad_full_s2_4rows': C(lambda: wgrad(1, 64, 64, 17, 17, stride=2, pad=0), ['conv_wgrad_full_kernel<3, 3, 2, 4>'], ['conv_wgrad_packed_kernel']),
    'wgrad_full_s2_2rows': C(lambda: wgrad(1, 64, 64, 17, 33, stride=2, pad=0), ['conv_wgrad_full_kernel<3, 3, 2, 2>'], ['conv_wgrad_packed_kernel']),
    'wgrad_full_s2_whole_chunks': C(lambda: wgrad(1, 64, 64, 9, 65, stride=2, pad=0), ['conv_wgrad_full_kernel<3, 3, 2, 1>'], ['conv_wgrad_kernel']),
    'wgrad_full_s2_partial_chunk': C(lambda: wgrad(1, 64, 64, 9, 63, stride=2, pad=0), ['conv_wgrad_kernel<3, 3, 2, 1>'], ['conv_wgrad_full_kernel']),
    'wgrad_masked_s2_ragged_i': C(lambda: wgrad(1, 48, 64, 9, 65, stride=2, pad=0), ['conv_wgrad_kernel<3, 3, 2, 1>'], ['conv_wgrad_full_kernel']),
    'wgrad_masked_s2_ragged_o': C(lambda: wgrad(1, 64, 40, 9, 65, stride=2, pad=0), ['conv_wgrad_kernel<3, 3, 2, 1>'], ['conv_wgrad_full_kernel']),
    'wgrad_full_1x1_one_row': C(lambda: wgrad(2, 64, 64, 8, 8, k=1, pad=0), ['conv_wgrad_full_kernel<1, 1, 1, 1>'], ['conv_wgrad_kernel', 'wgrad_thin_kernel']),
    'wgrad_masked_1x1_ragged': C(lambda: wgrad(2, 72, 24, 8, 8, k=1, pad=0), ['conv_wgrad_kernel<1, 1, 1, 1>'], ['conv_wgrad_full_kernel', 'wgrad_thin_kernel']),
    'wgrad_masked_1x1_partial_row': C(lambda: wgrad(2, 64, 64, 5, 13, k=1, pad=0), ['conv_wgrad_kernel<1, 1, 1, 1>'], ['conv_wgrad_full_kernel']),
    'wgrad_1x1_stride2': C(lambda: wgrad(1, 16, 16, 8, 8, k=1, stride=2, pad=0), ['conv_wgrad_kernel<1, 1, 2, 1>'], ['wgrad_thin_kernel']),
    'wgrad_thin_4x4': C(lambda: wgrad(1, 3, 32, 64, 64, k=1, pad=0), ['wgrad_thin_kernel<4, 4>', 'wgrad_reduce_kernel<1>'], ['conv_wgrad_kernel']),
    'wgrad_thin_4x1': C(lambda: wgrad(1, 3, 32, 32, 32, k=1, pad=0), ['wgrad_thin_kernel<4, 1>', 'wgrad_reduce_kernel<1>'], ['conv_wgrad_kernel']),
    'wgrad_thin_8x4': C(lambda: wgrad(1, 8, 32, 64, 64, k=1, pad=0), ['wgrad_thin_kernel<8, 4>'], ['conv_wgrad_kernel']),
    'wgrad_thin_8x1_toRGB_side': C(lambda: wgrad(1, 32, 5, 32, 32, k=1, pad=0), ['wgrad_thin_kernel<8, 1>'], ['conv_wgrad_kernel']),
    'wgrad_thin_unaligned': C(lambda: wgrad(1, 3, 32, 32, 32, k=1, pad=0, offset=True), ['conv_wgrad_kernel<1, 1, 1, 1>'], ['wgrad_thin_kernel']),
    'wgrad_reduce_2': C(lambda: wgrad(8, 3, 32, 32, 32, k=1, pad=0), ['wgrad_thin_kernel<4, 1>', 'wgrad_reduce_kernel<2>'], []),
    'wgrad_reduce_4': C(lambda: wgrad(16, 3, 32, 32, 32, k=1, pad=0), ['wgrad_thin_kernel<4, 1>', 'wgrad_reduce_kernel<4>'], []),
    'wgrad_reduce_8': C(lambda: wgrad(32, 3, 32, 32, 32, k=1, pad=0), ['wgrad_thin_kernel<4, 1>', 'wgrad_reduce_kernel<8>'], []),
    'wgrad_reduce_16': C(lambda: wgrad(64, 3, 32, 32, 32, k=1, pad=0), ['wgrad_thin_kernel<4, 1>', 'wgrad_reduce_kernel<16>'], []),
    # ---- upfirdn2d: row-marching separable kernels, the 4x4 'same' kernel, the generic kernel
    'fir_pad2_march_k1': C(lambda: fir(2, 3, 16, 64), [f'{FDM}<1, 8, 0>'], ['fir_same_kernel', 'upfirdn_generic_kernel']),
    'fir_pad2_march_k2': C(lambda: fir(1, 2, 9, 128, flip=True, gain=0.37), [f'{FDM}<2, 8, 0>'], ['fir_same_kernel']),
    'fir_pad2_march_k4': C(lambda: fir(1, 2, 9, 256), [f'{FDM}<4, 8, 0>'], ['fir_same_kernel', 'fir_down_march4_kernel']),
    'fir_pad2_march_k8': C(lambda: fir(1, 2, 5, 512), [f'{FDM}<8, 4, 0>'], ['fir_same_kernel']),
    'fir_pad2_march_k1_w16': C(lambda: fir(3, 5, 10, 16), [f'{FDM}<1, 8, 0>'], ['fir_same_kernel']),
    'fir_pad2_unsupported_w48': C(lambda: fir(2, 3, 16, 48), ['fir_same_kernel<4, 4, true>'], [FDM]),
    'fir_pad2_march_off': C(lambda: fir(2, 3, 16, 64), ['fir_same_kernel<4, 4, true>'], [FDM], {'FIR_MARCH': False}),
    'fir_same_nonsep_vec4': C(lambda: fir(2, 3, 16, 64, sep=False), ['fir_same_kernel<4, 4, true>'], [FDM]),
    'fir_same_w_mod4_2': C(lambda: fir(2, 3, 16, 18, sep=False), ['fir_same_kernel<4, 4, false>'], ['fir_same_kernel<4, 4, true>']),
    'fir_same_x_unaligned': C(lambda: fir(2, 3, 16, 64, sep=False, offset=True), ['fir_same_kernel<4, 4, false>'], ['fir_same_kernel<4, 4, true>']),
    'fir_same_pad5': C(lambda: fir(2, 3, 16, 64, pad=(5, 1, 1, 1), sep=False), ['fir_same_kernel<4, 4, false>'], ['fir_same_kernel<4, 4, true>']),
    'fir_dn2_march_k1': C(lambda: fir(2, 3, 16, 64, down=2, pad=(1, 1, 1, 1)), ['fir_dn2_march_kernel<1>'], ['upfirdn_generic_kernel']),
    'fir_dn2_march_k2': C(lambda: fir(1, 2, 8, 512, down=2, pad=(1, 1, 1, 1)), ['fir_dn2_march_kernel<2>'], ['upfirdn_generic_kernel']),
    'fir_up2_march_k1': C(lambda: fir(2, 3, 7, 64, up=2, pad=(2, 1, 2, 1)), ['fir_up2_march_kernel<1>'], ['upfirdn_generic_kernel']),
    'fir_up2_march_k2': C(lambda: fir(1, 2, 5, 256, up=2, pad=(2, 1, 2, 1), flip=True), ['fir_up2_march_kernel<2>'], ['upfirdn_generic_kernel']),
    'fir_dn2_nonsep_generic': C(lambda: fir(2, 3, 16, 64, down=2, pad=(1, 1, 1, 1), sep=False), ['upfirdn_generic_kernel'], ['fir_dn2_march_kernel']),
    'fir_dn2_unaligned_generic': C(lambda: fir(2, 3, 16, 64, down=2, pad=(1, 1, 1, 1), offset=True), ['upfirdn_generic_kernel'], ['fir_dn2_march_kernel']),
    'fir_dn2_unsupported_w40': C(lambda: fir(2, 3, 16, 40, down=2, pad=(1, 1, 1, 1)), ['upfirdn_generic_kernel'], ['fir_dn2_march_kernel']),
    'fir_up2_unsupported_w96': C(lambda: fir(2, 3, 8, 96, up=2, pad=(2, 1, 2, 1)), ['upfirdn_generic_kernel'], ['fir_up2_march_kernel']),
    'fir_up2_march_off': C(lambda: fir(2, 3, 7, 64, up=2, pad=(2, 1, 2, 1)), ['upfirdn_generic_kernel'], ['fir_up2_march_kernel'], {'FIR_MARCH': False}),
    'fir_strided_f32': C(lambda: fir_strided(torch.float32), ['upfirdn_strided_kernel<float, float>'], []),
    'fir_strided_f64': C(lambda: fir_strided(torch.float64), ['upfirdn_strided_kernel<double, double>'], []),
    'fir_strided_f16': C(lambda: fir_strided(torch.float16), [('upfirdn_strided_kernel<_Float16, float>', '_Z22upfirdn_strided_kernelIDF16_f')], []),
    # ---- upfir_planar: separable marching kernel, generic kernel (vector / scalar stores, 32 / 64 / 128-column tiles)
    'upfir_sep_march_12': C(lambda: upfir_planar(2, 3, 8, 32), ['fir_up_march_kernel<1, 2>'], ['fir_up_planar_kernel']),
    'upfir_sep_march_21': C(lambda: upfir_planar(1, 2, 8, 256), ['fir_up_march_kernel<2, 1>'], ['fir_up_planar_kernel']),
    'upfir_sep_residual_unaligned': C(lambda: upfir_planar(2, 3, 8, 32, res_offset=True), ['fir_up_planar_kernel<false, 32>'], ['fir_up_march_kernel']),
    'upfir_sep_unsupported_w48': C(lambda: upfir_planar(2, 3, 8, 48), ['fir_up_planar_kernel<true, 64>'], ['fir_up_march_kernel']),
    'upfir_sep_march_off': C(lambda: upfir_planar(2, 3, 8, 32), ['fir_up_planar_kernel<true, 32>'], ['fir_up_march_kernel'], {'FIR_MARCH': False}),
    'upfir_generic_v32': C(lambda: upfir_planar(2, 3, 8, 16, sep=False), ['fir_up_planar_kernel<true, 32>'], ['fir_up_march_kernel']),
    'upfir_generic_s32': C(lambda: upfir_planar(2, 3, 8, 17, sep=False), ['fir_up_planar_kernel<false, 32>'], ['fir_up_march_kernel']),
    'upfir_generic_v64': C(lambda: upfir_planar(2, 3, 8, 64, sep=False), ['fir_up_planar_kernel<true, 64>'], ['fir_up_march_kernel']),
    'upfir_generic_s64': C(lambda: upfir_planar(2, 3, 8, 49, sep=False), ['fir_up_planar_kernel<false, 64>'], ['fir_up_march_kernel']),
    'upfir_generic_v128': C(lambda: upfir_planar(2, 3, 8, 128, sep=False, epi=False), ['fir_up_planar_kernel<true, 128>'], ['fir_up_march_kernel']),
    'upfir_generic_s128': C(lambda: upfir_planar(2, 3, 8, 97, sep=False), ['fir_up_planar_kernel<false, 128>'], ['fir_up_march_kernel']),
    # ---- bias_act: float4 kernel when HW % 4 == 0 and x / y / noise / residual are 16-byte aligned, the scalar kernel otherwise
    'bias_act_v4': C(lambda: bias_act(), ['bias_act_v4_kernel'], ['bias_act_kernel']),
    'bias_act_v4_noise_shared_res': C(lambda: bias_act(noise='shared', res=True), ['bias_act_v4_kernel'], ['bias_act_kernel']),
    'bias_act_v4_noise_per_sample': C(lambda: bias_act(noise='per', res=True, act=False), ['bias_act_v4_kernel'], ['bias_act_kernel']),
    'bias_act_v4_plain': C(lambda: bias_act(scale=False, bias=False), ['bias_act_v4_kernel'], ['bias_act_kernel']),
    'bias_act_hw_mod4': C(lambda: bias_act(h=15, w=15, noise='per', res=True), ['bias_act_kernel'], ['bias_act_v4_kernel']),
    'bias_act_x_unaligned': C(lambda: bias_act(x_off=True, noise='shared', res=True), ['bias_act_kernel'], ['bias_act_v4_kernel']),
    'bias_act_x_16B_not_32B': C(lambda: bias_act(x_off=4, noise='per', res=True), ['bias_act_v4_kernel'], ['bias_act_kernel']),
    'bias_act_noise_unaligned': C(lambda: bias_act(noise='shared', noise_off=True, res=True), ['bias_act_kernel'], ['bias_act_v4_kernel']),
    'bias_act_noise_per_unaligned': C(lambda: bias_act(noise='per', noise_off=True, act=False), ['bias_act_kernel'], ['bias_act_v4_kernel']),
    'bias_act_residual_unaligned': C(lambda: bias_act(noise='per', res=True, res_off=True), ['bias_act_kernel'], ['bias_act_v4_kernel']),
    'bias_act_clamp_v4': C(lambda: bias_act_clamp(16), ['bias_act_v4_kernel'], ['bias_act_kernel']),
    'bias_act_clamp_scalar': C(lambda: bias_act_clamp(15), ['bias_act_kernel'], ['bias_act_v4_kernel']),
    'bias_act_backward_clamp': C(lambda: bias_act_bwd(True), ['bias_act_backward_kernel'], []),
    'bias_act_backward_linear': C(lambda: bias_act_bwd(False), ['bias_act_backward_kernel'], []),
    # ---- toRGB: the quad kernel for O <= 3, W % 4 == 0, aligned, small or large grids; the pixel kernel otherwise
    'torgb4': C(lambda: torgb(2, 32, 3, 16, 16), ['torgb4_kernel'], ['torgb_kernel']),
    'torgb4_base_up': C(lambda: torgb(2, 32, 3, 16, 16, base=True), ['torgb4_kernel'], ['torgb_kernel']),
    'torgb_o4': C(lambda: torgb(2, 32, 4, 16, 16), ['torgb_kernel<4>'], ['torgb4_kernel']),
    'torgb_o4_base_up': C(lambda: torgb(2, 32, 4, 16, 16, base=True), ['torgb_kernel<4>'], ['torgb4_kernel']),
    'torgb_mid_grid_base_up': C(lambda: torgb(2, 8, 3, 256, 256, base=True), ['torgb_kernel<4>'], ['torgb4_kernel']),
    'torgb_w_mod4': C(lambda: torgb(2, 32, 3, 16, 18), ['torgb_kernel<4>'], ['torgb4_kernel']),
    # ---- minibatch standard deviation
    'mbstd_group_4': C(lambda: mbstd(8, 16, 4, 4, 4), ['mbstd_stat_kernel', 'mbstd_write_kernel'], []),
    'mbstd_group_2_f2': C(lambda: mbstd(8, 16, 4, 4, 2, f=2), ['mbstd_stat_kernel', 'mbstd_write_kernel'], []),
    'mbstd_group_none': C(lambda: mbstd(6, 16, 4, 4, None), ['mbstd_stat_kernel', 'mbstd_write_kernel'], []),
    'mbstd_group_clamped_to_n': C(lambda: mbstd(3, 16, 4, 4, 4), ['mbstd_stat_kernel', 'mbstd_write_kernel'], []),
}


def _flat(out):
    if isinstance(out, (list, tuple)):
        return torch.cat([t.reshape(-1) for t in out])
    return out


def _ok(pattern, names):
    alts = pattern if isinstance(pattern, tuple) else (pattern,)
    return any(any_hit(p, names) if not p.startswith('_Z') else any(p in n for n in names) for p in alts)


@pytest.mark.parametrize('case', sorted(CASES))
def test_route(case):
    kk = _kk()
    builder, expect, forbid, switches = CASES[case]
    old = {k: getattr(kk, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(kk, k, v)
        call, ref, tol = builder()
        alts = [p for p in expect if not isinstance(p, tuple)]
        got, names = launched(call, expect=alts)
    finally:
        for k, v in old.items():
            setattr(kk, k, v)
    kern = sorted(n for n in names if 'kernel' in n)
    for p in expect:
        assert _ok(p, names), f'{case}: expected {p} to run; ran {kern}'
    for p in forbid:
        assert not any_hit(p, names), f'{case}: {p} must not run; ran {kern}'
    got = _flat(got).detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (case, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), case
    e = rel_err(got.numpy(), ref.numpy())
    print(f'ROUTE {case} rel_err={e:.3e}')
    if tol == 0.0:
        assert torch.equal(got, ref), f'{case}: not bit-exact (rel err {e:.3e})'
    else:
        assert e < tol, f'{case}: rel err {e:.3e} >= {tol:.0e}'


# Every kernel launched from conv_mfma.hip, conv_wino.hip, conv_wino4.hip, conv_wino_poly.hip, conv_wgrad.hip, conv_wgrad_wino.hip,
# upfirdn2d.hip and the float32 part of pointwise.hip (their hipLaunchKernelGGL sites), with the instantiation where the site picks one.
ROUTE_KERNELS = [
    S1_DB, S1_NARROW, S1_WIDE, S2_DB, S2_NARROW, S2_WIDE, UP_RAW_N, UP_RAW_W, UP_EPI_N, UP_EPI_W, UP_SMALL, C1_N, C1_W, MSPLIT,
    'conv1x1_gemm_kernel<1, 4, 16>', 'conv1x1_gemm_kernel<2, 2, 16>',
    f'{WINO}<4, 16>', f'{WINO}<8, 8>', WSPLIT,
    f'{WINO4}<1, 32>', f'{WINO4}<2, 16>', f'{WINO4}<4, 8>',
    f'{POLY_UP}<8, 8, 0, 8, 8>', f'{POLY_UP}<1, 64, 11, 4, 16>', f'{POLY_UP}<1, 64, 22, 4, 16>', f'{POLY_UP}<1, 64, 43, 4, 16>',
    f'{POLY_UP}<4, 16, 0, 4, 16>', f'{POLY_UP}<8, 8, 0, 4, 16>',
    f'{POLY_DOWN}<2, 1, 64, 11>', f'{POLY_DOWN}<2, 1, 64, 22>', f'{POLY_DOWN}<2, 1, 64, 43>', f'{POLY_DOWN}<2, 4, 16, 0>',
    f'{POLY_DOWN}<2, 8, 8, 0>', f'{POLY_DOWN}<3, 2, 32, 0>', f'{POLY_DOWN}<3, 4, 16, 0>', f'{POLY_DOWN}<3, 8, 8, 0>',
    'wgrad_reduce_kernel<1>', 'wgrad_reduce_kernel<2>', 'wgrad_reduce_kernel<4>', 'wgrad_reduce_kernel<8>', 'wgrad_reduce_kernel<16>',
    'wgrad_thin_kernel<4, 4>', 'wgrad_thin_kernel<4, 1>', 'wgrad_thin_kernel<8, 4>', 'wgrad_thin_kernel<8, 1>',
    'conv_wgrad_packed_kernel<3, 3, 1>', 'conv_wgrad_packed_kernel<3, 3, 2>', 'conv_wgrad_kernel<3, 3, 1, 2>',
    'conv_wgrad_full_kernel<3, 3, 2, 2>', 'conv_wgrad_full_kernel<3, 3, 2, 4>', 'conv_wgrad_full_kernel<3, 3, 2, 1>',
    'conv_wgrad_full_kernel<1, 1, 1, 1>', 'conv_wgrad_kernel<3, 3, 1, 1>', 'conv_wgrad_kernel<3, 3, 2, 1>', 'conv_wgrad_kernel<1, 1, 1, 1>',
    'conv_wgrad_kernel<1, 1, 2, 1>',
    f'{WGW}<3>', f'{WGW}<2>', f'{WGW}<1>', f'{WGW}<0>',
    'fir_same_kernel<4, 4, true>', 'fir_same_kernel<4, 4, false>', 'upfirdn_generic_kernel',
    'upfirdn_strided_kernel<float, float>', 'upfirdn_strided_kernel<_Float16, float>', 'upfirdn_strided_kernel<double, double>',
    'fir_down_march4_kernel<1, 8, 0>', 'fir_down_march4_kernel<2, 8, 0>',
    f'{FDM}<1, 8, 0>', f'{FDM}<2, 8, 0>', f'{FDM}<4, 8, 0>', f'{FDM}<8, 4, 0>',
    'fir_up_planar_kernel<true, 128>', 'fir_up_planar_kernel<false, 128>', 'fir_up_planar_kernel<true, 64>', 'fir_up_planar_kernel<false, 64>',
    'fir_up_planar_kernel<true, 32>', 'fir_up_planar_kernel<false, 32>',
    'fir_up_march_kernel<1, 2>', 'fir_up_march_kernel<2, 1>',
    'fir_dn2_march_kernel<1>', 'fir_dn2_march_kernel<2>', 'fir_up2_march_kernel<1>', 'fir_up2_march_kernel<2>',
    'bias_act_v4_kernel', 'bias_act_kernel', 'bias_act_backward_kernel', 'conv1x1_small_i_kernel<8>', 'torgb4_kernel', 'torgb_kernel<4>',
    'mbstd_stat_kernel', 'mbstd_write_kernel',
]

# launched from those files but left out of the table, and why
NOT_ROUTED = {
    'weight_scale_kernel / weight_transpose_kernel / weight_sq_kernel (conv_mfma.hip), wino_weight_kernel, wino4_weight_kernel, '
    'poly_weight_kernel': 'weight preparation: one kernel per layout, no choice; every convolution case above consumes its output',
    'splitk_reduce_kernel, wino_split_reduce_kernel past their grid caps; the fix launch of conv_mfma_kernel': 'routed above at '
    'one trip; their second trips, ragged slices and the tail split are loop bounds, held in test_gpu_loop_bounds_fp32.py',
    'fma_kernel, fma_bcast_kernel<float|double>, mul_reduce_kernel<float|double>': 'one kernel per dtype, no shape or alignment '
    'dispatch; their grid caps, reduction tails and stride plans are held to float64 in test_gpu_pointwise_edges.py (the plans on the host in '
    'test_pointwise_plan_cpu.py)',
    'planes_to_image_kernel, modtail_backward_f32_kernel, scale_cast_to_half_kernel, scale_cast_to_float_kernel, sum_partials_kernel, '
    'scale_channels_kernel, composite_u8_kernel, assemble_input_kernel, assemble_input_u8_kernel': 'single-kernel entry points without a '
    'route choice; their grid caps, loop remainders, channel slices and argument checks are held to float64 in test_gpu_pointwise_edges.py',
    'float16 kernels of pointwise.hip and conv_f16*.hip': 'the fp16 entry points have a route table of their own, test_gpu_routes_fp16.py (every '
    'launch site of conv_f16*.hip by kernel name, both sides of each predicate, against float64)',
}


def _key(p):
    return p[0] if isinstance(p, tuple) else p


def test_route_table_covers_every_kernel():
    """Every kernel / instantiation the float32 entry points can launch is the expected route of at least one case (host-only: no launch)."""
    expected = {_key(p).replace(' ', '') for _, (_, exp, _, _) in CASES.items() for p in exp}
    missing = [k for k in ROUTE_KERNELS if k.replace(' ', '') not in expected]
    assert not missing, f'kernels without a route case: {missing}'
    assert len(set(ROUTE_KERNELS)) == len(ROUTE_KERNELS)
