"""CPU (gloo, world size 2): the streamed evaluation loop ``eval_harness.EvalLoop`` -- lib/experiments/shgan_default.py:264-300 with
the collectives of SURVEY 8(e): per-batch nothing, at the end one all-gather of the uint8 results + zipzap and one all-reduce of the
FID moments -- and ``broadcast_state``, the rank-0 checkpoint load + weight broadcast of shgan_default.py:138-154,223-231.  The
generator step and the moment kernel need a GPU; stand-ins are injected for both (the product forms run in tests/test_gpu_eval_loop.py)."""
import os
import subprocess
import sys

import torch

from conftest import ROOT


def _run_two(script, port_base):
    port = str(port_base + os.getpid() % 2000)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), SHG_ROOT=ROOT, SHG_PORT=port)
        procs.append(subprocess.Popen([sys.executable, '-c', script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=240)
        assert p.returncode == 0, out.decode()


def test_gloo_world2_eval_loop_streams_gathers_and_reduces_moments():
    script = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"])
import shgan_amd
from shgan_amd import eval_harness as hz, data
from shgan_amd.fid_stats import FidStats
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
R, N, B, D = 32, 11, 4, 16
def step(x, z, out):                       # stand-in generator step writing INTO the loop's result buffer
    img = torch.tanh(x[:, 1:4] * 0.5 + z[:, :3, None, None] * 0.1)
    m = x[:, 0:1] + 0.5
    out.copy_(((x[:, 1:4] * m + img * (1 - m)) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8))
    return out
def acc(S, feats, w):                      # stand-in for the fp64-MFMA moment kernel: the same augmented second moments
    f = torch.cat([feats.double(), torch.ones(feats.shape[0], 1, dtype=torch.float64)], 1)
    if w is not None:
        S[:D + 1, :D + 1] += (f * w.double()[:, None]).t() @ f
    else:
        S[:D + 1, :D + 1] += f.t() @ f
def latents(ids, b):
    g = torch.Generator()
    out = torch.empty(b, 8)
    for k, i in enumerate(ids):
        g.manual_seed(100 + int(i)); out[k].normal_(generator=g)
    return out
def masks_for(ids):
    return torch.stack([((torch.arange(R * R).reshape(R, R) * (int(i) + 3)) % 7 > 2).float() for i in ids])
class Loader:
    def __init__(self, ids): self.ids = ids
    def __iter__(self):
        inner = hz.PinnedU8Loader(self.ids, B, R, seed=5)
        for img, ids in inner:
            yield img, masks_for(ids), ids
feat = lambda u8: hz.standin_features(u8, D)
def run(rank, world):
    loop = hz.EvalLoop(None, "cpu", R, N, rank=rank, world=world, noise_mode="const", feature_fn=feat, fid_dim=D, latent_fn=latents,
                       device_masks=False, step_fn=step, fid_accumulate_fn=acc)
    seen = []
    loop.on_batch = lambda ids, out, ev: seen.append(list(ids))
    loop.run(Loader(loop.ids))
    assert sum(len(s) for s in seen) == len(loop.ids) and [i for s in seen for i in s] == loop.ids
    return loop
loop = run(r, 2)
assert loop.ids == ([0, 2, 4, 6, 8, 10] if r == 0 else [1, 3, 5, 7, 9, 0])
images, fid = loop.gather()
assert images.shape == (N, 3, R, R) and images.dtype == torch.uint8
# the same evaluation on one rank without a process group's help: built by hand from the pieces
one = hz.EvalLoop(None, "cpu", R, N, rank=0, world=1, noise_mode="const", feature_fn=feat, fid_dim=D, latent_fn=latents, device_masks=False,
                  step_fn=step, fid_accumulate_fn=acc)
one.run(Loader(one.ids))
assert torch.equal(images, one.images), "gathered + zipzapped result != the 1-rank run"
# zipzap on the device == the reference's host re-interleave
full = torch.stack([run(q, 2).images for q in range(2)])
assert np.array_equal(hz.zipzap_device(full, N).numpy(), data.zipzap_arrange([full[0].numpy(), full[1].numpy()])[:N])
# moments: the padded duplicate (item 0 on rank 1) has weight 0, so the all-reduced sum equals the 1-rank sum and counts N samples
n2, mu2, sg2 = fid.mean_cov()
n1, mu1, sg1 = one.local_fid().mean_cov()
assert n2 == n1 == N, (n2, n1)
assert np.allclose(mu2, mu1, rtol=0, atol=1e-12) and np.allclose(sg2, sg1, rtol=0, atol=1e-9)
dist.destroy_process_group()
print("rank", r, "ok")
'''
    _run_two(script, 33500)


def test_gloo_world2_broadcast_state_from_rank0():
    script = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"])
import shgan_amd
from shgan_amd import eval_harness as hz
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(7, 5)
        self.b = torch.nn.Conv2d(3, 4, 3)
        self.register_buffer("avg", torch.zeros(5))
        self.register_buffer("steps", torch.zeros((), dtype=torch.int64))
torch.manual_seed(10 + r)                  # the ranks start DIFFERENT: only rank 0 "read the checkpoint"
net = Net()
if r == 0:
    net.avg.fill_(0.25); net.steps.fill_(12345)
ref = Net(); torch.manual_seed(10); ref2 = Net(); ref2.avg.fill_(0.25); ref2.steps.fill_(12345)
v0 = {k: p._version for k, p in net.named_parameters()}
nbytes = hz.broadcast_state(net, src=0)
want = sum(t.numel() * 4 for t in list(net.parameters()) + [net.avg]) + 8
assert nbytes == want, (nbytes, want)
for (k, t), (_, u) in zip(sorted(net.state_dict().items()), sorted(ref2.state_dict().items())):
    assert t.dtype == u.dtype and torch.equal(t, u), k
assert all(p._version > v0[k] for k, p in net.named_parameters()), "parameters must be written through copy_ (version counters move)"
dist.destroy_process_group()
print("rank", r, "ok")
'''
    _run_two(script, 35500)


def test_broadcast_state_without_a_process_group_is_a_no_op():
    import torch
    import shgan_amd  # noqa: F401
    from shgan_amd import eval_harness as hz
    net = torch.nn.Linear(3, 2)
    w = net.weight.detach().clone()
    assert hz.broadcast_state(net) == 0 and torch.equal(net.weight, w)


# ---- every option on at once: the order of the calls inside a batch and of the collectives at the end

ALL_ON = dict(R=16, N=11, B=4, D=64, C=9, SPLITS=3, PR_DIM=6, KID=dict(num_subsets=4, max_subset_size=6, seed=3))
# what a batch does on its stream, in order (the KID copies and the writes into the buffers are plain tensor copies: no stand-in sees them)
BATCH_CALLS = ['step', ('detector', None, True), 'is_accumulate', 'fid_accumulate', ('detector', 'pm1', False), 'fid_accumulate', 'metrics',
               'lpips', ('pr_detector', None), ('pr_detector', 'pm1')]


def all_on_loop(rank, world, log):
    """EvalLoop on the CPU with every option on and a stand-in for every kernel; each stand-in appends its name to ``log`` (detectors:
    with the ``input_range`` they were given), the generator step first."""
    import kid_is_f64
    import pr_f64
    from shgan_amd import eval_harness as hz
    R, N, B, D, C = (ALL_ON[k] for k in ('R', 'N', 'B', 'D', 'C'))

    def step(x, z, out):
        log.append('step')
        out.copy_(((x[:, 1:4] * 0.5 + z[:, :3, None, None] * 0.2).tanh() * 127.5 + 127.5).clamp(0, 255).to(torch.uint8))
        return out

    def values(img, input_range):
        return img.float() * 127.5 + 127.5 if input_range == 'pm1' else img.float()
    W = torch.randn(C, D, generator=torch.Generator().manual_seed(1)) * 0.05

    class Det:
        num_classes = C

        def __call__(self, img, input_range=None, with_probs=False):
            log.append(('detector', input_range, with_probs))
            f = hz.standin_features(values(img, input_range), D) / 64
            # (one matrix-vector product per image: the same bits whatever batch the image arrives in)
            return (f, torch.softmax(torch.stack([W @ fi for fi in f]), 1)) if with_probs else f

    class PrDet:
        dim = ALL_ON['PR_DIM']

        def __call__(self, img, input_range=None):
            log.append(('pr_detector', input_range))
            return hz.standin_features(values(img, input_range), self.dim) / 64

    def fid_acc(S, feats, w):
        log.append('fid_accumulate')
        f = torch.cat([feats.double(), torch.ones(feats.shape[0], 1, dtype=torch.float64)], 1)
        S[:D + 1, :D + 1] += (f * w.double()[:, None]).t() @ f

    def is_acc(a, probs, splits):
        log.append('is_accumulate')
        a += torch.from_numpy(kid_is_f64.is_accumulator_f64(probs.numpy(), splits.numpy(), a.shape[0]))

    def diff(pred, real):
        return pred.double() / 255 - (real.double() + 1) / 2

    def metrics_fn(pred, gt, ws, p_out, s_out):
        log.append('metrics')
        p_out.copy_(diff(pred, gt).pow(2).mean(dim=(1, 2, 3)))
        s_out.copy_(diff(pred, gt).abs().amax(dim=(1, 2, 3)))

    def lpips(pred, real, out=None):
        log.append('lpips')
        out.copy_(diff(pred, real).abs().mean(dim=(1, 2, 3)))

    def latents(ids, b):
        g, out = torch.Generator(), torch.empty(b, 8)
        for k, i in enumerate(ids):
            g.manual_seed(100 + int(i))
            out[k].normal_(generator=g)
        return out

    def loader(ids):
        for b0 in range(0, len(ids), B):
            g, imgs = torch.Generator(), []
            for i in ids[b0:b0 + B]:
                g.manual_seed(7000 + int(i))
                imgs.append(torch.rand(3, R, R, generator=g) * 2 - 1)
            yield torch.stack(imgs), torch.ones(len(imgs), R, R) * (torch.arange(R) % 3 > 0).float(), ids[b0:b0 + B]
    pr_fns = (lambda f, k: torch.from_numpy(pr_f64.radii16(f.numpy(), k)),
              lambda p, m, r: torch.from_numpy(pr_f64.inside16(p.numpy(), m.numpy(), r.numpy())))
    loop = hz.EvalLoop(None, 'cpu', R, N, rank=rank, world=world, noise_mode='const', feature_fn=Det(), fid_dim=D, latent_fn=latents,
                       device_masks=False, step_fn=step, fid_accumulate_fn=fid_acc, metrics=('psnr', 'ssim'), ssim_window=7,
                       metrics_fn=metrics_fn, fid_real=True, lpips=lpips, kid=dict(ALL_ON['KID'], sums_fn=kid_is_f64.kid_sums_f64),
                       inception_score=dict(num_splits=ALL_ON['SPLITS'], accumulate_fn=is_acc),
                       pr=dict(detector=PrDet(), nhood_size=2, kernels_fn=pr_fns))
    loop.run(loader(loop.ids))
    return loop


def test_every_option_on_one_rank_calls_in_order_per_batch():
    """11 items in batches of 4 (a ragged last batch), every option on: each batch makes exactly the calls of BATCH_CALLS, in that order."""
    import shgan_amd  # noqa: F401
    log = []
    loop = all_on_loop(0, 1, log)
    assert log == BATCH_CALLS * 3
    images, fid = loop.gather()
    assert log == BATCH_CALLS * 3                                       # gather runs no stand-in
    N, D = ALL_ON['N'], ALL_ON['D']
    assert images.shape == (N, 3, 16, 16) and fid is loop.fid and fid.mean_cov()[0] == N == loop.fid_real.mean_cov()[0]
    assert [t.shape for t in loop.kid_features] == [(N, D)] * 2 and [t.shape for t in loop.pr_features] == [(N, ALL_ON['PR_DIM'])] * 2
    assert float(loop.is_acc[:, -1].sum()) == N
    assert sorted(loop.image_metrics) == ['lpips', 'lpips_per_image', 'psnr', 'psnr_per_image', 'ssim', 'ssim_per_image']
    assert torch.equal(loop.image_metrics['lpips_per_image'], loop.lpips_values)
    for fn in (loop.fid_value, loop.kid_value, loop.is_value, loop.pr_value):
        fn()


def test_gloo_world2_every_option_on_collectives_in_order():
    """World 2: the per-batch calls are those of one rank; ``gather`` issues one collective per result, in the order every rank relies
    on; what it returns equals the 1-rank run (bit for bit where rows are only moved; sums of float64 terms taken in another order --
    moments, Inception Score accumulators, means -- within 1e-12 relative)."""
    script = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["SHG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SHG_ROOT"], "tests"))
import shgan_amd
from test_eval_loop_cpu import ALL_ON, BATCH_CALLS, all_on_loop
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["SHG_PORT"], rank=int(os.environ["RANK"]), world_size=2)
r = dist.get_rank()
N, D, C, S, P = (ALL_ON[k] for k in ("N", "D", "C", "SPLITS", "PR_DIM"))
seen = []
def record(name):
    fn = getattr(dist, name)
    def wrapped(*args, **kw):
        t = args[1] if name == "all_gather_into_tensor" else args[0]           # the rank's own contribution
        seen.append((name, t.dtype, tuple(t.shape)))
        return fn(*args, **kw)
    setattr(dist, name, wrapped)
record("all_gather_into_tensor"); record("all_reduce")
log = []
loop = all_on_loop(r, 2, log)
assert log == BATCH_CALLS * 2 and not seen                                     # 6 items per rank: batches of 4 and 2; no collective per batch
images, fid = loop.gather()
dp = (D + 1 + 31) // 32 * 32
gather, reduce = "all_gather_into_tensor", "all_reduce"
assert seen == [(gather, torch.uint8, (6, 3, 16, 16)), (reduce, torch.float64, (dp, dp)), (reduce, torch.float64, (dp, dp)),
                (gather, torch.float64, (6, 3)), (gather, torch.float32, (6, D)), (gather, torch.float32, (6, D)),
                (gather, torch.float16, (6, P)), (gather, torch.float16, (6, P)), (reduce, torch.float64, (S, C + 2))], seen
values = (loop.fid_value(), loop.kid_value(), loop.is_value(), loop.pr_value())
dist.destroy_process_group()
one = all_on_loop(0, 1, [])
images1, fid1 = one.gather()
assert torch.equal(images, images1)
for a, b in zip(loop.kid_features + loop.pr_features, one.kid_features + one.pr_features):
    assert a.dtype == b.dtype and torch.equal(a, b)
assert sorted(loop.image_metrics) == sorted(one.image_metrics)
for k, v in one.image_metrics.items():
    if torch.is_tensor(v):
        assert torch.equal(loop.image_metrics[k], v), k
    else:
        assert abs(loop.image_metrics[k] - v) <= 1e-12 * abs(v), k
close = lambda a, b: bool(np.allclose(np.asarray(a), np.asarray(b), rtol=1e-12, atol=0))
assert close(fid.S, fid1.S) and close(loop.fid_real.S, one.fid_real.S) and close(loop.is_acc, one.is_acc)
assert float(fid.S[D, D]) == N == float(loop.is_acc[:, -1].sum())              # the padded duplicate on rank 1 counts nowhere
want = (one.fid_value(), one.kid_value(), one.is_value(), one.pr_value())
assert values[1] == want[1] and values[3] == want[3]
assert abs(values[0] - want[0]) <= 1e-9 * max(1.0, abs(want[0])) and close(values[2], want[2])
print("rank", r, "ok")
"""
    _run_two(script, 43500)
