"""Build recipe for libshgan_hip.so (gfx950 only, hipcc, in-tree output).

``python sh-gan_amd/build.py`` or ``__graft_entry__.build()``.  hipcc cross-compiles without a GPU.
The shared object is linked WITHOUT an rpath to /opt/rocm so that, inside a PyTorch-ROCm process,
it binds to the HIP runtime torch has already loaded (one runtime per process)."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIBDIR = os.path.join(HERE, 'lib')
LIB = os.path.join(LIBDIR, 'libshgan_hip.so')
SOURCES = ['capi.hip', 'upfirdn2d.hip', 'pointwise.hip', 'dense.hip', 'conv_mfma.hip', 'conv_wino.hip', 'conv_wino4.hip', 'conv_wino_poly.hip', 'conv_wgrad.hip', 'conv_wgrad_wino.hip', 'conv_f16.hip', 'conv_wgrad_f16.hip', 'upfirdn2d_f16.hip', 'pointwise_f16.hip', 'conv_f16_ring.hip', 'conv_f16_upring.hip', 'conv_f16_down.hip', 'shu.hip', 'mask_raster.hip', 'mask_lama.hip', 'fid_stats.hip', 'image_metrics.hip', 'resize.hip', 'randcrop.hip', 'ada.hip', 'ada_tail.hip', 'inception.hip', 'lpips.hip', 'lpips_bwd.hip', 'optim.hip', 'kid.hip', 'pr.hip', 'vgg16.hip', 'ppl.hip', 'plural.hip', 'svm.hip', 'gemm_f64.hip', 'inpaint.hip', 'membrane.hip', 'hole_label.hip', 'train_stats.hip']
# per-source extras: the Winograd weight-gradient transforms are scalar fp32 chains beside MFMAs -- SLP-packed (v_pk_*) forms cost register
# moves and issue slots there
SRC_FLAGS = {'conv_wgrad_wino.hip': ['-fno-slp-vectorize']}
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc', '-Wall', '-Wno-unused-function', '-Wno-inline-asm']


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError('hipcc not found')


INCLUDE = os.path.join(os.path.dirname(HERE), 'include')


def _digest():
    """sha256 over every kernel source, the public C header (an ABI struct edit must trigger a rebuild) and the flags."""
    h = hashlib.sha256()
    for d in (CSRC, INCLUDE):
        for name in sorted(os.listdir(d)):
            with open(os.path.join(d, name), 'rb') as fh:
                h.update(name.encode())
                h.update(fh.read())
    h.update(' '.join(list(FLAGS) + [f'{k}:{v}' for k, v in sorted(SRC_FLAGS.items())]).encode())
    return h.hexdigest()


def build(force=False, verbose=True):
    os.makedirs(LIBDIR, exist_ok=True)
    stamp = os.path.join(LIBDIR, '.build_digest')
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read().strip() == dig:
        if verbose:
            print(f'[build] {os.path.basename(LIB)} up to date')
        return LIB
    hipcc = _hipcc()
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(LIBDIR, src.replace('.hip', '.o'))
        objs.append(obj)
        cmd = [hipcc] + FLAGS + SRC_FLAGS.get(src, []) + ['-c', os.path.join(CSRC, src), '-o', obj]
        if verbose:
            print('[build]', ' '.join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            sys.stderr.write(out.decode(errors='replace'))
            raise RuntimeError(f'hipcc failed on {src}')
        if verbose and out.strip():
            print(out.decode(errors='replace'))
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
    if verbose:
        print('[build]', ' '.join(cmd))
    subprocess.check_call(cmd)
    for obj in objs:
        os.remove(obj)
    with open(stamp, 'w') as fh:
        fh.write(dig)
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
