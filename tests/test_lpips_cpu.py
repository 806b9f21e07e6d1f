"""CPU (no GPU): LPIPS's host side (sh-gan_amd/lpips.py, csrc/lpips.hip) -- the float64 model of tests/lpips_f64.py against an
independently assembled ``torch.nn`` stack, the two weight layouts and their validation, the operand value tables, the C ABI's argument
checks and export list, and ``EvalLoop(lpips=...)``'s dataset-order bookkeeping over a gloo world of two with torch stand-ins."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
from conftest import ROOT
from shgan_amd import _lib, kernels, lpips

import lpips_f64 as ref
from test_image_metrics_cpu import _run_two

NEW = ('shg_lpips_conv1_weight_prep_f32', 'shg_lpips_conv1_f32', 'shg_lpips_head_scratch_bytes', 'shg_lpips_head_f32')
TV_INDEX = (0, 3, 6, 8, 10)


def _alexnet_features():
    """torchvision's ``alexnet().features``, restated layer by layer at its indices."""
    nn = torch.nn
    return nn.Sequential(nn.Conv2d(3, 64, 11, stride=4, padding=2), nn.ReLU(), nn.MaxPool2d(3, 2),
                         nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(), nn.MaxPool2d(3, 2),
                         nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(), nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(),
                         nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(), nn.MaxPool2d(3, 2))


def _two_files(sd):
    alex = {}
    for (key, *_), i in zip(ref.CONVS, TV_INDEX):
        alex[f'features.{i}.weight'], alex[f'features.{i}.bias'] = sd[f'{key}.weight'], sd[f'{key}.bias']
    alex.update({'classifier.1.weight': torch.zeros(4096, 9216), 'classifier.1.bias': torch.zeros(4096), 'classifier.6.weight': torch.zeros(1000, 4096)})
    lin = {k: v for k, v in sd.items() if k.startswith('lin')}
    return alex, lin


def test_float64_model_equals_an_independent_torch_nn_stack():
    sd = ref.random_state_dict(3)
    feats = _alexnet_features().double()
    feats.load_state_dict({f'{i}.{p}': sd[f'{key}.{p}'].double() for (key, *_), i in zip(ref.CONVS, TV_INDEX) for p in ('weight', 'bias')})
    lins = [torch.nn.Conv2d(c, 1, 1, bias=False).double() for c in (64, 192, 384, 256, 256)]
    for n, m in enumerate(lins):
        m.load_state_dict({'weight': sd[f'lin{n}.model.1.weight'].double()})
    pred_u8, real_u8 = ref.image_pairs(3, 72, 90, seed=1)
    real = real_u8.float().div(255) * 2 - 1
    in0 = torch.from_numpy((((pred_u8.numpy() / 255) - 0.5) * 2).astype(np.float32)).double()
    in1 = ((((real + 1) / 2) - 0.5) * 2).double()
    shift = torch.tensor([-.030, -.088, -.188]).double()[None, :, None, None]
    scale = torch.tensor([.458, .448, .450]).double()[None, :, None, None]
    x0, x1, total = (in0 - shift) / scale, (in1 - shift) / scale, 0
    k = 0
    for i, layer in enumerate(feats):
        x0, x1 = layer(x0), layer(x1)
        if i in (1, 4, 7, 9, 11):
            n0 = x0 / (torch.sqrt(torch.sum(x0 ** 2, dim=1, keepdim=True)) + 1e-10)
            n1 = x1 / (torch.sqrt(torch.sum(x1 ** 2, dim=1, keepdim=True)) + 1e-10)
            total = total + lins[k]((n0 - n1) ** 2).mean([2, 3], keepdim=True)
            k += 1
    want = total.flatten()
    got = ref.lpips_f64(sd, pred_u8, real)
    assert k == 5 and got.shape == (3,) and float(got.min()) > 1e-4
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12
    assert torch.equal(ref.lpips_f64(sd, pred_u8, real_u8), got)                 # decoded uint8 reals: the same values
    x = torch.rand(2, 3, 40, 40)
    assert torch.equal(ref.lpips_f64(sd, x, x, 'unit'), torch.zeros(2, dtype=torch.float64))


def test_both_weight_layouts_load_to_the_same_tensors():
    sd = ref.random_state_dict(5)
    a = lpips.canonical_weights(sd)
    b = lpips.canonical_weights(*_two_files(sd))
    assert list(a) == list(b) and len(a) == 17
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].dtype == torch.float32, k
    assert torch.equal(a['shift'], torch.tensor(lpips.SHIFT)) and torch.equal(a['scale'], torch.tensor(lpips.SCALE))
    assert a['lin2'].shape == (384,) and a['conv0.weight'].shape == (64, 3, 11, 11)
    full = dict(sd, **{f'lins.{k}.model.1.weight': sd[f'lin{k}.model.1.weight'] for k in range(5)})
    full['scaling_layer.shift'] = torch.tensor([-.03, -.09, -.19]).reshape(1, 3, 1, 1)
    full['scaling_layer.scale'] = torch.tensor([.45, .44, .46]).reshape(1, 3, 1, 1)
    c = lpips.canonical_weights(full)
    assert torch.equal(c['shift'], torch.tensor([-.03, -.09, -.19])) and torch.equal(c['scale'], torch.tensor([.45, .44, .46]))
    assert torch.equal(c['lin4'], a['lin4'])
    assert lpips.macs_per_pair(512, 512) == 2 * (127 * 127 * 64 * 363 + 63 * 63 * 192 * 1600 + 31 * 31 * (384 * 1728 + 256 * 3456 + 256 * 2304))
    assert 7.2e9 < lpips.macs_per_pair(512, 512) < 7.4e9


def test_validation_errors_name_the_key():
    E = _lib.ShgError
    sd = ref.random_state_dict(0)
    lpips.validate_state_dict(sd)
    miss = {k: v for k, v in sd.items() if k != 'net.slice3.6.bias'}
    with pytest.raises(E, match=r"lacks 'net\.slice3\.6\.bias'"):
        lpips.validate_state_dict(miss)
    with pytest.raises(E, match=r"unexpected.*'net\.slice6\.12\.weight'"):
        lpips.validate_state_dict(dict(sd, **{'net.slice6.12.weight': torch.zeros(1)}))
    with pytest.raises(E, match=r"'lin1\.model\.1\.weight' has shape \(1, 64, 1, 1\), expected \(1, 192, 1, 1\)"):
        lpips.validate_state_dict(dict(sd, **{'lin1.model.1.weight': torch.zeros(1, 64, 1, 1)}))
    with pytest.raises(E, match=r"'scaling_layer\.shift' has shape"):
        lpips.validate_state_dict(dict(sd, **{'scaling_layer.shift': torch.zeros(3)}))
    with pytest.raises(E, match=r"'lins\.2\.model\.1\.weight' differs"):
        lpips.canonical_weights(dict(sd, **{'lins.2.model.1.weight': torch.ones(1, 384, 1, 1)}))
    alex, lin = _two_files(sd)
    lpips.validate_state_dicts(alex, lin)
    with pytest.raises(E, match=r"alexnet state_dict lacks 'features\.8\.weight'"):
        lpips.validate_state_dicts({k: v for k, v in alex.items() if k != 'features.8.weight'}, lin)
    with pytest.raises(E, match=r"unexpected alexnet state_dict key 'avgpool\.weight'"):
        lpips.validate_state_dicts(dict(alex, **{'avgpool.weight': torch.zeros(1)}), lin)
    with pytest.raises(E, match=r"lin state_dict lacks 'lin4\.model\.1\.weight'"):
        lpips.validate_state_dicts(alex, {k: v for k, v in lin.items() if k != 'lin4.model.1.weight'})
    with pytest.raises(E, match=r"unexpected lin state_dict key 'net\.slice1\.0\.weight'"):
        lpips.validate_state_dicts(alex, dict(lin, **{'net.slice1.0.weight': sd['net.slice1.0.weight']}))
    # validation comes before any device is touched
    with pytest.raises(E, match=r"net\.slice1\.0\.weight"):
        lpips.Lpips.from_state_dict({k: v for k, v in sd.items() if k != 'net.slice1.0.weight'}, device='cpu')
    with pytest.raises(E, match=r"features\.0\.bias"):
        lpips.Lpips.from_state_dicts({k: v for k, v in alex.items() if k != 'features.0.bias'}, lin, device='cpu')


def test_value_tables_equal_the_evaluator_batch_bit_for_bit():
    """All 256 codes, both operands, against a numpy restatement of shgan_default.py:283-286 + eva_lpips.py:39-45."""
    codes = np.arange(256, dtype=np.uint8)
    fake = codes / 255                                         # numpy: float64
    pred = torch.Tensor(((fake - 0.5) * 2)).float()            # eva_lpips.py:39,43
    assert torch.equal(lpips.value_table_cpu('pred'), pred) and pred.dtype == torch.float32
    real = kernels.u8_value_table('cpu')                       # the dataset route's float32 real in [-1, 1]
    gt = (real.numpy().astype(np.float32) + np.float32(1)) / np.float32(2)
    assert gt.dtype == np.float32
    gt = (gt - np.float32(0.5)) * np.float32(2)
    assert gt.dtype == np.float32 and np.array_equal(lpips.value_table_cpu('gt', 'pm1').numpy(), gt)
    unit = ((codes / 255).astype(np.float32) - np.float32(0.5)) * np.float32(2)
    assert np.array_equal(lpips.value_table_cpu('gt', 'unit').numpy(), unit)
    # the helper the GPU tests use forms the same values
    u8 = torch.from_numpy(codes).reshape(1, 1, 16, 16)
    assert torch.equal(ref.pred_values_f32(u8).flatten(), pred) and np.array_equal(ref.gt_values_f32(u8).flatten().numpy(), gt)
    assert np.array_equal(ref.gt_values_f32(u8, 'unit').flatten().numpy(), unit)
    assert np.array_equal(ref.gt_values_f32(real.reshape(1, 1, 16, 16)).flatten().numpy(), gt)


def test_abi_argument_checks_reject_bad_calls_without_a_gpu():
    lib = _lib.get_lib()
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    p, f3 = ctypes.c_void_p(16), (ctypes.c_float * 3)(.458, .448, .450)

    def c1(x=p, shift=f3, scaling=f3, wp=p, bp=p, y=p, B=2, H=64, W=64):
        return lib.shg_lpips_conv1_f32(x, None, 1.0, 0.0, shift, scaling, wp, bp, y, B, H, W, None)
    for kw in ({'x': None}, {'shift': None}, {'scaling': None}, {'wp': None}, {'bp': None}, {'y': None}):
        assert c1(**kw) == -1 and 'null' in err(), kw
    assert c1(wp=ctypes.c_void_p(8)) == -1 and 'aligned' in err()
    for kw in ({'B': 0}, {'H': 6}, {'W': 6}, {'H': -1}):
        assert c1(**kw) == -1 and 'geometry' in err(), kw
    assert c1(scaling=(ctypes.c_float * 3)(.458, 0.0, .450)) == -1 and 'scale of 0' in err()
    assert lib.shg_lpips_conv1_weight_prep_f32(None, p, p, p, None) == -1 and 'null' in err()
    assert lib.shg_lpips_conv1_weight_prep_f32(p, p, p, None, None) == -1

    def hd(fp=p, fg=p, w=p, B=2, C=64, h=15, wd=15, scratch=p, nbytes=1 << 20, out=p):
        return lib.shg_lpips_head_f32(fp, fg, w, B, C, h, wd, scratch, nbytes, out, None)
    for kw in ({'fp': None}, {'fg': None}, {'w': None}, {'scratch': None}, {'out': None}):
        assert hd(**kw) == -1 and 'null' in err(), kw
    for kw in ({'B': 0}, {'C': 0}, {'h': 0}, {'wd': -2}):
        assert hd(**kw) == -1 and '>= 1' in err(), kw
    need = lib.shg_lpips_head_scratch_bytes(2, 15, 15)
    assert need == 2 * 4 * 8                                   # one float64 per 64-pixel tile and image
    assert hd(nbytes=need - 1) == -1 and 'too small' in err()
    assert lib.shg_lpips_head_scratch_bytes(16, 127, 127) == 16 * 253 * 8
    assert lib.shg_lpips_head_scratch_bytes(0, 15, 15) == 0 and lib.shg_lpips_head_scratch_bytes(1, 0, 15) == 0


def test_exports_signatures_and_abi_number():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert 'eva_lpips.py' in hdr and 'SHG_LPIPS_CONV1_WP_ELEMS (368 * 64)' in hdr
    assert _lib.ABI_VERSION == 40 and _lib.get_lib().shg_abi_version() == 40     # symbols were added, nothing changed
    assert _lib.get_lib().shg_lpips_head_scratch_bytes.restype == ctypes.c_size_t


def test_python_api_refuses_host_tensors_small_images_and_bad_operands():
    E = _lib.ShgError
    net = lpips.Lpips(None, [], [], lpips.SHIFT, lpips.SCALE, 'cpu')
    x = torch.zeros(1, 3, 64, 64, dtype=torch.uint8)
    with pytest.raises(E, match='device'):
        net(x, torch.zeros(1, 3, 64, 64))
    with pytest.raises(E, match='gt_range'):
        net(x, x, gt_range='01')
    with pytest.raises(E, match='one shape'):
        net(x, torch.zeros(1, 3, 64, 32))
    with pytest.raises(E, match='device'):
        lpips.conv1(x, None, None)
    with pytest.raises(E, match='device'):
        lpips.head(torch.zeros(1, 4, 3, 3), torch.zeros(1, 4, 3, 3), torch.zeros(4), torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match='callable'):
        from shgan_amd import eval_harness as hz
        hz.EvalLoop(None, 'cpu', 8, 4, lpips=3)
    assert lpips.out_sizes(31) == (7, 3, 1, 1, 1) and lpips.out_sizes(512) == (127, 63, 31, 31, 31) and lpips.MIN_SIZE == 31


def test_gloo_world2_eval_loop_lpips_in_dataset_order():
    script = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SHG_ROOT"], "tests"))
import shgan_amd
from shgan_amd import eval_harness as hz
from test_image_metrics_cpu import reference_metrics_f64
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
R, N, B = 24, 11, 4
def step(x, z, out):
    img = torch.tanh(x[:, 1:4] * 0.5 + z[:, :3, None, None] * 0.1)
    m = x[:, 0:1] + 0.5
    res = ((x[:, 1:4] * m + img * (1 - m)) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8)
    return res if out is None else out.copy_(res)
def standin(pred, real):                     # a per-pair number with the network's signature; it measures nothing
    p = pred.to(torch.float64) / 255 * 2 - 1
    g = (real.to(torch.float64) / 255 * 2 - 1) if real.dtype == torch.uint8 else real.to(torch.float64)
    d = (p - g).abs()
    return d.mean(dim=(1, 2, 3)) + 0.25 * d[:, :, ::3, ::3].amax(dim=(1, 2, 3))
calls = []
def lp(pred, real, out=None):
    calls.append(pred.shape[0])
    assert out.dtype == torch.float64 and out.shape == (pred.shape[0],) and bool(torch.isnan(out).all())
    out.copy_(standin(pred, real))
def mfn(pred, gt, ws, p_out, s_out):
    p, s = reference_metrics_f64(pred, gt, ws)
    if p_out is not None: p_out.copy_(p)
    if s_out is not None: s_out.copy_(s)
def latents(ids, b):
    g = torch.Generator(); out = torch.empty(b, 8)
    for k, i in enumerate(ids):
        g.manual_seed(100 + int(i)); out[k].normal_(generator=g)
    return out
def masks_for(ids):
    return torch.stack([((torch.arange(R * R).reshape(R, R) * (int(i) + 3)) % 7 > 2).float() for i in ids])
class Loader:
    def __init__(self, ids): self.ids = ids
    def __iter__(self):
        for img, ids in hz.PinnedU8Loader(self.ids, B, R, seed=5):
            yield img, masks_for(ids), ids
def run(rank, world, keep=True, metrics=None, lpips=lp):
    loop = hz.EvalLoop(None, "cpu", R, N, rank=rank, world=world, noise_mode="const", latent_fn=latents, device_masks=False, step_fn=step,
                       keep_images=keep, metrics=metrics, ssim_window=7, metrics_fn=mfn, lpips=lpips)
    loop.run(Loader(loop.ids))
    return loop
# lpips alone
loop = run(r, 2)
images, fid = loop.gather()
im = loop.image_metrics
assert fid is None and sorted(im) == ["lpips", "lpips_per_image"], sorted(im)
assert im["lpips_per_image"].shape == (N,) and im["lpips_per_image"].dtype == torch.float64
assert calls == [4, 2] and loop.lpips_values.shape == (6,) and not bool(torch.isnan(loop.lpips_values).any())
# the 1-rank run, item by item in dataset order
one = run(0, 1)
assert one.ids == list(range(N)) and torch.equal(one.lpips_values, im["lpips_per_image"])
# the values belong to the items: recomputed from the gathered images and the loader's pixels in dataset order
real = hz.PinnedU8Loader(list(range(N)), N, R, seed=5)._draw(list(range(N)))
want = standin(images, real)
assert torch.equal(want, im["lpips_per_image"])
# the mean is over exactly n_items: the padded duplicate (item 0 again, on rank 1) is not counted
assert im["lpips"] == float(want.mean())
assert abs(im["lpips"] - float(torch.cat([want, want[:1]]).mean())) > 1e-9
# with metrics: one table, PSNR / SSIM as without lpips; without the image gather too
both = run(r, 2, keep=False, metrics=("psnr", "ssim"))
imgs2, _ = both.gather()
assert imgs2 is None and both.images is None
assert sorted(both.image_metrics) == ["lpips", "lpips_per_image", "psnr", "psnr_per_image", "ssim", "ssim_per_image"]
assert torch.equal(both.image_metrics["lpips_per_image"], im["lpips_per_image"])
plain = run(r, 2, metrics=("psnr", "ssim"), lpips=None)
plain.gather()
assert sorted(plain.image_metrics) == ["psnr", "psnr_per_image", "ssim", "ssim_per_image"]
for k in plain.image_metrics:
    a, b = plain.image_metrics[k], both.image_metrics[k]
    assert torch.equal(a, b) if torch.is_tensor(a) else a == b, k
# off: no call, nothing set
calls.clear()
off = run(r, 2, lpips=None)
off.gather()
assert not calls and off.image_metrics is None and off.lpips_values is None
dist.destroy_process_group()
print("rank", r, "ok")
'''
    _run_two(script, 41500)
