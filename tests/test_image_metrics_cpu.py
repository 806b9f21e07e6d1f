"""CPU (no GPU): the image-quality evaluators (sh-gan_amd/image_metrics.py; reference lib/evaluator/eva_psnr.py, eva_ssim.py) --
the C ABI's argument checks, the float64 restatement the GPU tests compare against (pinned here on the reference's own outputs,
tests/golden/image_metrics.npz from tools/gen_golden_metrics.py), and the dataset-order bookkeeping of ``EvalLoop(metrics=...)``
over a gloo world of two with torch stand-ins for the generator step and the metric kernel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden


def reference_metrics_f64(pred, gt, window_size=11, gt_range='pm1'):
    """Float64 restatement of eva_psnr (for_dataset=None, rgb_range=1) and eva_ssim._ssim (size_average=False) on the CPU: pred / gt
    in the forms ``image_metrics`` takes (uint8 or float32; gt in [-1, 1] for 'pm1').  The SSIM window is create_window's (float32
    taps, float32 outer product), the arithmetic float64.  -> (psnr [B], ssim [B]) float64."""
    from shgan_amd import kernels
    from shgan_amd.image_metrics import pred_value_table

    def val(t, table):                 # the operand's float32 value
        t = t.cpu()
        return table[t.long()] if t.dtype == torch.uint8 else t.to(torch.float32)
    pred = pred.cpu()
    # PSNR: the composite's pixels as numpy float64 u8 / 255, gt = (real + 1) / 2 rounded to float32 (the evaluator batch's forms)
    x = pred.to(torch.float64) / 255 if pred.dtype == torch.uint8 else pred.to(torch.float64)
    y = ((val(gt, kernels.u8_value_table('cpu')) + 1) / 2 if gt_range == 'pm1' else val(gt, pred_value_table('cpu'))).to(torch.float64)
    psnr = -10 * torch.log10(((x - y) ** 2).mean(dim=(1, 2, 3)))
    # SSIM: both operands as float32 (torch.FloatTensor in eva_ssim.add_batch), arithmetic in float64
    x = val(pred, pred_value_table('cpu')).to(torch.float64)
    c = x.shape[1]
    ws, r = int(window_size), int(window_size) // 2
    g = torch.tensor([np.exp(-(k - r) ** 2 / float(2 * 1.5 ** 2)) for k in range(ws)], dtype=torch.float32)
    g = g / g.sum()
    win = (g[:, None] @ g[None, :]).to(torch.float64).expand(c, 1, ws, ws).contiguous()

    def flt(v):
        return F.conv2d(v, win, padding=r, groups=c)
    mu1, mu2 = flt(x), flt(y)
    s1, s2, s12 = flt(x * x) - mu1 * mu1, flt(y * y) - mu2 * mu2, flt(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return psnr, m.mean(dim=(1, 2, 3))


def golden_cases():
    gd = load_golden('image_metrics')
    for name in gd['cases']:
        name = str(name)
        real_u8 = gd[name + '/real_u8']
        yield (name, torch.from_numpy(gd[name + '/pred_u8']), torch.from_numpy(real_u8),
               torch.from_numpy(real_u8).to(torch.float32).div(255) * 2 - 1, int(gd[name + '/window']), gd[name + '/psnr'], gd[name + '/ssim'])


def test_float64_restatement_matches_the_reference_evaluators():
    n = 0
    for name, pred_u8, real_u8, real, ws, psnr_ref, ssim_ref in golden_cases():
        for gt in (real, real_u8):             # the feeder's float32 real and the decoded pixels give the same values
            psnr, ssim = reference_metrics_f64(pred_u8, gt, ws)
            assert np.abs(psnr.numpy() - psnr_ref).max() <= 1e-9, name
            assert np.abs(ssim.numpy() - ssim_ref).max() <= 2e-6, name
        n += 1
    assert n == 5


def _args(lib, pred=8, gt=8, scratch=8, psnr=8, ssim=8, B=2, C=3, H=16, W=16, ws=11, nbytes=1 << 20, psnr_only=0):
    p = ctypes.c_void_p
    return lib.shg_image_metrics(p(pred) if pred else None, None, 1.0, 0.0, p(gt) if gt else None, None, 0.5, 0.5, B, C, H, W, ws, psnr_only,
                                 p(scratch) if scratch else None, nbytes, p(psnr) if psnr else None, p(ssim) if ssim else None, None)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from shgan_amd import _lib
    lib = _lib.get_lib()
    for kw in ({'pred': 0}, {'gt': 0}, {'scratch': 0}, {'psnr': 0}, {'ssim': 0}):
        assert _args(lib, **kw) == -1 and b'null' in lib.shg_last_error(), kw
    for ws in (0, 2, 10, 12, 33, -1):
        assert _args(lib, ws=ws) == -1 and b'window_size' in lib.shg_last_error(), ws
        assert lib.shg_image_metrics_scratch_bytes(2, 16, 16, ws) == 0
    for kw in ({'B': 0}, {'C': 0}, {'H': 0}, {'W': -3}):
        assert _args(lib, **kw) == -1 and b'>= 1' in lib.shg_last_error(), kw
    need = lib.shg_image_metrics_scratch_bytes(2, 16, 16, 11)
    assert need > 0 and need % 16 == 0
    assert _args(lib, nbytes=need - 1) == -1 and b'too small' in lib.shg_last_error()
    # one fp64 (squared error, SSIM) pair per tile and image; the scratch grows with the tile count
    assert lib.shg_image_metrics_scratch_bytes(16, 512, 512, 11) == 16 * (512 // 64) * (512 // 16) * 16
    assert lib.shg_image_metrics_scratch_bytes(1, 1, 1, 31) == 16
    # PSNR alone needs no SSIM output
    assert _args(lib, ssim=0, psnr_only=1, nbytes=need - 1) == -1 and b'too small' in lib.shg_last_error()


def test_python_api_refuses_cpu_tensors_and_even_windows():
    from shgan_amd._lib import ShgError as E
    from shgan_amd.image_metrics import MetricsAccumulator, image_metrics
    x = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(E, match='device'):
        image_metrics(x, torch.zeros(1, 3, 8, 8))
    with pytest.raises(E, match='window_size'):
        image_metrics(x, torch.zeros(1, 3, 8, 8), window_size=10)
    with pytest.raises(E, match='subset'):
        MetricsAccumulator(4, 'cpu', metrics=('lpips',))


def _run_two(script, port_base):
    port = str(port_base + os.getpid() % 2000)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), SHG_ROOT=ROOT, SHG_PORT=port)
        procs.append(subprocess.Popen([sys.executable, '-c', script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=240)
        assert p.returncode == 0, out.decode()


def test_gloo_world2_eval_loop_metrics_in_dataset_order():
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
calls = []
def mfn(pred, gt, ws, p_out, s_out):         # stand-in for the HIP launch pair: the float64 restatement, written into the slices
    calls.append(pred.shape[0])
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
def run(rank, world, keep=True, metrics=("psnr", "ssim")):
    loop = hz.EvalLoop(None, "cpu", R, N, rank=rank, world=world, noise_mode="const", latent_fn=latents, device_masks=False, step_fn=step,
                       keep_images=keep, metrics=metrics, ssim_window=7, metrics_fn=mfn)
    loop.run(Loader(loop.ids))
    return loop
loop = run(r, 2)
images, fid = loop.gather()
assert fid is None and images.shape == (N, 3, R, R)
im = loop.image_metrics
assert sorted(im) == ["psnr", "psnr_per_image", "ssim", "ssim_per_image"], sorted(im)
assert im["psnr_per_image"].shape == (N,) and im["ssim_per_image"].shape == (N,) and im["psnr_per_image"].dtype == torch.float64
# the 1-rank run, item by item in dataset order
one = run(0, 1)                            # (inside the world-2 group: its local values are the 1-rank result, ids 0..N-1)
assert one.ids == list(range(N))
assert torch.equal(one.metrics.values["psnr"], im["psnr_per_image"])
assert torch.equal(one.metrics.values["ssim"], im["ssim_per_image"])
# the values belong to the items: recomputed from the gathered images and the loader's pixels in dataset order
real = hz.PinnedU8Loader(list(range(N)), N, R, seed=5)._draw(list(range(N)))
p, s = reference_metrics_f64(images, real, 7)
assert torch.equal(p, im["psnr_per_image"]) and torch.equal(s, im["ssim_per_image"])
# means over exactly n_items: the padded duplicate (item 0 again, on rank 1) is not counted
assert im["psnr"] == float(p.mean()) and im["ssim"] == float(s.mean())
assert abs(im["psnr"] - float(torch.cat([p, p[:1]]).mean())) > 1e-9
# without the image gather: the same values
lean = run(r, 2, keep=False, metrics=("ssim",))
imgs2, _ = lean.gather()
assert imgs2 is None and lean.images is None
assert sorted(lean.image_metrics) == ["ssim", "ssim_per_image"] and torch.equal(lean.image_metrics["ssim_per_image"], im["ssim_per_image"])
# metrics off: no metric call, no attribute set
calls.clear()
off = run(r, 2, metrics=None)
off.gather()
assert not calls and off.image_metrics is None
dist.destroy_process_group()
print("rank", r, "ok")
'''
    _run_two(script, 37500)
