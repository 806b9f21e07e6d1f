"""Dataset side of the hot path: FFHQ zip listing, PNG decode, the CoModGAN mask formatter, and the hand-off
of host batches to the device input of the generator.

Mirrors ``lib/data_factory/ds_ffhq.py``:
  * ``ffhqzip_list``          -- ``ffhqzip.init_load_info`` :262-305: the PNG members of ``ffhq{256x256,512x512}.zip`` sorted by
    unique id, ``simple_split`` [0, 10000) = validation, [10000, 70000) = training;
  * ``ZipLoader``             -- :307-330: one open ``ZipFile`` per worker, PNG bytes -> uint8 HWC -> float CHW / 255
    (``torchvision.transforms.ToTensor``).  The reference decodes with ``pyspng``; Pillow yields the same pixels;
  * ``RandomMaskFormatter``   -- :332-347: ``x = image * 2 - 1``, horizontal flip with probability 1/2, ``RandomMask`` -- in this order of
    ``numpy.random`` draws, so a seeded worker produces the reference's sample stream;
  * ``LamaMaskFormatter``     -- :352-381: the same with the LaMa thin / medium / thick masks (``data.LamaMask``; on the device:
    ``masks.lama_masks``, ``DeviceFeeder(mask_kind='lama_thin', device_masks=True)``).  The reference draws these with ``cv2.line``; the
    rasteriser here is a restatement of OpenCV's algorithm, not checked against ``cv2`` itself;
  * ``FFHQZip``               -- the ``ds_base.__getitem__`` composition (element -> loader -> formatter);
  * ``DeviceFeeder``          -- what ``shgan_default.py:267-274`` does per batch (``x = cat([mask - 0.5, real * mask])``), on the device:
    pinned staging, H2D on a copy stream overlapped with the previous batch's kernels, masks either from the host formatter or
    drawn on the device (``masks.random_masks``, bit-identical to the host implementation), ``assemble_input`` kernel.

Training input of Places2, OpenImages and DTD: ``draw_scale_crop`` makes the draws of the reference's "random scale, random crop"
formatters (``AdvInpaintingFormatter``, ds_places2.py:183-207 / ds_openimages.py:117-141; ``InpaintingFormatter``, ds_texture.py:121-149)
on the host, items carry them as 'crop', and ``DeviceFeeder`` computes the window on the device (``resize.randcrop_bicubic``); ``Texture``
is the DTD dataset of ds_texture.py."""
import io
import os
from zipfile import ZipFile

import numpy as np
import numpy.random as npr
import torch

from . import data as _data

_MODES = {
    'train256': ('ffhq256x256.zip', (10000, 70000)), 'val256': ('ffhq256x256.zip', (0, 10000)),
    'train512': ('ffhq512x512.zip', (10000, 70000)), 'train512ori': ('ffhq512x512.zip', (10000, 70000)),
    'val512': ('ffhq512x512.zip', (0, 10000)), 'val512ori': ('ffhq512x512.zip', (0, 10000)),
}


def ffhqzip_list(root_dir, mode):
    """load_info of ``ffhqzip`` (ds_ffhq.py:262-305)."""
    if mode not in _MODES:
        raise ValueError(mode)
    zipname, split = _MODES[mode]
    zpath = os.path.join(root_dir, zipname)
    info = []
    with ZipFile(zpath, 'r') as z:
        for fi in z.namelist():
            if fi.find('.png') == -1:
                continue
            filename = os.path.basename(fi)
            info.append({'unique_id': os.path.splitext(filename)[0], 'filename': filename, 'image_path': fi, 'zipfile': zpath})
    info = sorted(info, key=lambda x: x['unique_id'])
    info = info[split[0]:split[1]]
    for idx, e in enumerate(info):
        e['idx'] = idx
    return info


class ZipLoader:
    """ds_ffhq.py:307-330: element -> element with 'image' (float32 [C,H,W] in [0,1]) and 'imsize'."""

    def __init__(self):
        self.zipfile, self.zipfilename = None, None

    def decode_u8(self, element):
        """uint8 [H,W,C] of the element's PNG."""
        from PIL import Image
        if self.zipfilename != element['zipfile']:
            self.zipfile_close()
            self.zipfile, self.zipfilename = ZipFile(element['zipfile'], 'r'), element['zipfile']
        with self.zipfile.open(element['image_path'], 'r') as f:
            img = np.asarray(Image.open(io.BytesIO(f.read())))
        return img[:, :, None] if img.ndim == 2 else img

    def __call__(self, element):
        element = dict(element)
        u8 = self.decode_u8(element)
        element['image'] = torch.from_numpy(np.ascontiguousarray(u8.transpose(2, 0, 1))).to(torch.float32).div(255)   # ToTensor
        element['imsize'] = [int(u8.shape[0]), int(u8.shape[1])]
        return element

    def zipfile_close(self):
        if self.zipfile is not None:
            self.zipfile.close()
        self.zipfile, self.zipfilename = None, None


class ImageOnlyFormatter:
    """ds_ffhq.py:247-256."""

    def __init__(self, random_flip=False):
        self.random_flip = random_flip

    def __call__(self, element):
        x = element['image'] * 2 - 1
        if self.random_flip and npr.rand() < 0.5:
            x = x.flip(-1)
        return x, element['unique_id']


class RandomMaskFormatter:
    """ds_ffhq.py:332-347: (x in [-1,1], mask [s,s] float32 with 1 = known -- ``RandomMask(...)[0]``; the eval loop adds the channel axis, shgan_default.py:270 --, unique_id), s = ``mask_resolution`` which must equal the image resolution; the flip draw comes before the mask's."""

    def __init__(self, random_flip=True, mask_resolution=256, hole_range=(0, 1)):
        self.random_flip, self.mask_resolution, self.hole_range = random_flip, mask_resolution, list(hole_range)

    def __call__(self, element):
        x = element['image'] * 2 - 1
        if self.random_flip and npr.rand() < 0.5:
            x = x.flip(-1)
        mask = _data.RandomMask(self.mask_resolution, self.hole_range)[0]
        return x, mask, element['unique_id']


MASK_KINDS = ('freeform', 'lama_thin', 'lama_medium', 'lama_thick')


def _check_mask_kind(who, mask_kind):
    if mask_kind not in MASK_KINDS:
        raise ValueError(f'{who}: mask_kind must be one of {MASK_KINDS} (got {mask_kind!r})')
    return mask_kind


class LamaMaskFormatter:
    """ds_ffhq.py:352-381: (x in [-1,1], mask [s,s] float32 with 1 = known, unique_id) with the LaMa thin / medium / thick masks
    (lama_mask_utils.py: ``1 - MixedMaskGenerator(**setting)(x)[0]``); one ``npr.rand()`` flip draw when ``random_flip``, then the mask's
    draws.  Any (type, resolution) outside thin / medium / thick x 256 / 512 raises ``ValueError``, as in the reference.  The strokes are
    rasterised by ``data.LamaMask`` -- a restatement of OpenCV's thick line, not checked against ``cv2`` itself."""

    def __init__(self, random_flip=True, resolution=256, type='thin'):
        from . import masks as _masks
        if (type, resolution) not in _masks.LAMA_SETTINGS:
            raise ValueError(f'LamaMaskFormatter: no setting for type {type!r} at resolution {resolution!r}')
        self.random_flip, self.resolution, self.type = random_flip, resolution, type

    def __call__(self, element):
        x = element['image'] * 2 - 1
        if self.random_flip and npr.rand() < 0.5:
            x = x.flip(-1)
        mask = _data.LamaMask(self.resolution, self.type)[0]
        return x, mask, element['unique_id']


class FFHQZip(torch.utils.data.Dataset):
    """``ffhqzip`` + ``ZipLoader`` + a formatter (ds_base.__getitem__ without its cache / transform options).  ``mask_kind`` other than
    'freeform' (configs ``ffhqzip_val{256,512}_inpainting_lama{1,2,3}``) installs ``LamaMaskFormatter(random_flip=False, resolution of
    the mode, type)`` and takes no ``formatter`` of the caller's."""

    def __init__(self, root_dir, mode, formatter=None, try_sample=None, repeat=1, mask_kind='freeform'):
        if _check_mask_kind('FFHQZip', mask_kind) != 'freeform':
            if formatter is not None:
                raise ValueError('FFHQZip: pass either a formatter or a LaMa mask_kind, not both')
            formatter = LamaMaskFormatter(random_flip=False, resolution=512 if '512' in mode else 256, type=mask_kind[5:])
        self.load_info = ffhqzip_list(root_dir, mode)
        if try_sample is not None:
            self.load_info = self.load_info[:try_sample]
        self.loader, self.formatter, self.repeat = ZipLoader(), formatter, repeat

    def __len__(self):
        return len(self.load_info) * self.repeat

    def __getitem__(self, idx):
        element = self.loader(self.load_info[idx % len(self.load_info)])
        return element if self.formatter is None else self.formatter(element)


class DeviceFeeder:
    """Host batches -> generator inputs on the device.

        feeder = DeviceFeeder(device, resolution=512, device_masks=True)
        for x4, real, mask, ids in feeder(loader):      # loader yields (x [B,3,R,R] in [-1,1], mask [B,1,R,R] or None, ids)
            img = G(x=x4, z=..., c=...)                 # or RaggedU8Batch (Places2: images of their own sizes, resized on the device;
                                                        # OpenImages, ``fit``: resized to their boxes and padded, boxed masks)

    The H2D copies of batch k+1 run on a copy stream while batch k's kernels execute (pinned staging buffers, one event per batch);
    ``device_masks`` draws the freeform masks on the device instead of taking the formatter's (same distribution and, for the same
    numpy RNG state, the same bits: ``masks.random_masks``).  ``mask_kind`` = 'lama_thin' | 'lama_medium' | 'lama_thick' draws the LaMa
    masks of ``LamaMaskFormatter`` there instead (``masks.lama_masks``: one copy, one launch, no hole-count read); ``hole_range`` is
    then ignored -- the LaMa generator has no rejection loop -- and a batch with content boxes (OpenImages) is refused: the reference
    has no such config.  Host masks are staged as they come, whatever their kind."""

    def __init__(self, device, resolution, hole_range=(0, 1), device_masks=False, own_stream=True, mask_kind='freeform'):
        """``own_stream=False``: stage on the CALLER's stream instead of a copy stream -- for callers whose own stream carries nothing
        but this staging (EvalLoop: the generator runs on three side streams).  The copies still overlap with the generator (pinned
        source, asynchronous), the process stays within four HIP streams = the default number of hardware queues, and the mask
        rasteriser's hole-count read never queues behind a generator stream that happens to share a hardware queue with the copy
        stream (measured: a full pipeline drain every third batch, MEASUREMENTS.md round 6)."""
        self.device = torch.device(device)
        self.resolution, self.hole_range, self.device_masks = resolution, tuple(hole_range), device_masks
        self.mask_kind = _check_mask_kind('DeviceFeeder', mask_kind)
        if self.device.type == 'cuda' and not own_stream:
            self.copy_stream = None
            self._inline = True
        elif self.device.type == 'cuda':
            from .eval_harness import shared_streams
            self.copy_stream = shared_streams(self.device, 1, kind='copy')[0]       # one staging stream per process (see shared_streams)
        else:
            self.copy_stream = None

    def _to_device(self, t):
        if self.copy_stream is None and getattr(self, '_inline', False):
            return (t if t.is_pinned() else t.pin_memory()).to(self.device, non_blocking=True)
        if self.copy_stream is None:
            return t.to(self.device)
        if not t.is_pinned():
            t = t.pin_memory()
        with torch.cuda.stream(self.copy_stream):
            d = t.to(self.device, non_blocking=True)
        return d

    def _resize_on_device(self, batch):
        """RaggedU8Batch -> uint8 [B,3,R,R] on the device: the packed bytes are uploaded like any other input and resized
        (resize.resize_bicubic_u8, Pillow's bicubic bit for bit, then the flips; a ``fit`` batch: resize.resize_fit_pad_u8, resized
        to its boxes and padded) on the staging stream, behind their upload.  A batch with ``crop`` (the training formatters' random
        scale and crop) -> float32 [B,3,R,R] in [-1,1]: resize.randcrop_bicubic on the same stream, fed the packed bytes themselves
        (DTD) or the loader's resize (Places2, OpenImages: ``preresize``)."""
        from .resize import randcrop_bicubic, resize_bicubic_u8, resize_fit_pad_u8
        if self.device.type != 'cuda':
            raise ValueError('DeviceFeeder: ragged uint8 batches are resized on a HIP device (there is no host path)')
        data = self._to_device(batch.data)
        st = self.copy_stream if self.copy_stream is not None else torch.cuda.current_stream(self.device)
        if batch.crop is not None and not batch.preresize:           # DTD: the window straight from the images at their own sizes
            return randcrop_bicubic(data, batch.shapes, self.resolution, batch.crop, stream=st)
        fn = resize_fit_pad_u8 if batch.fit else resize_bicubic_u8
        u8 = fn(data, batch.shapes, self.resolution, flip=batch.flip, stream=st)
        if batch.crop is None:
            return u8
        return randcrop_bicubic(u8, None, self.resolution, batch.crop, stream=st)     # Places2 / OpenImages 'adv': the loader's resize first

    def _stage(self, batch):
        boxes = None
        if isinstance(batch, RaggedU8Batch):
            mask, ids = batch.masks, batch.ids
            if batch.fit and self.mask_kind != 'freeform':
                from ._lib import ShgError
                raise ShgError('DeviceFeeder: LaMa masks with content boxes (OpenImages) are not served: the reference has no such config')
            xd = self._resize_on_device(batch)
            x = xd
            if batch.fit and batch.crop is None:      # AdvInpaintingFormatter has no box fill (ds_openimages.py:129-141)
                boxes = np.asarray(batch.content_size, dtype=np.int32).reshape(-1, 2)
        else:
            x, mask, ids = (batch[0], batch[1], batch[2]) if len(batch) == 3 else (batch[0], None, batch[1])
            xd = self._to_device(x.contiguous())
        md = None
        if not self.device_masks:
            if mask is None:
                raise ValueError('DeviceFeeder: the loader yields no masks and device_masks is off')
            m = torch.as_tensor(np.asarray(mask), dtype=torch.float32)
            if m.ndim == 4 and m.shape[1] == 1:
                m = m[:, 0]
            if tuple(m.shape) != (x.shape[0], x.shape[2], x.shape[3]):
                raise ValueError(f'DeviceFeeder: masks {tuple(m.shape)} do not match the images {tuple(x.shape)} -- the formatter\'s '
                                 f'mask_resolution must equal the image resolution ({x.shape[2]}x{x.shape[3]})')
            if boxes is not None:                 # the formatter's box fill (idempotent on OpenImages' host masks, which carry it)
                m = m.clone()
                for k, box in enumerate(boxes):
                    fill_outside_box(m[k], box)
            md = self._to_device(m[:, None].contiguous())
        ev = None
        if self.copy_stream is not None:
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return xd, md, ids, ev, boxes

    def _finish(self, staged):
        from . import eval_harness, masks as _masks
        xd, md, ids, ev, boxes = staged
        if ev is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            xd.record_stream(cur)
            if md is not None:
                md.record_stream(cur)
        if md is None and self.mask_kind != 'freeform':
            # on the caller's stream, behind the wait above: nothing reads the device back, so there is nothing to keep off this stream
            md, _ = _masks.lama_masks(xd.shape[0], self.resolution, self.mask_kind, device=self.device)
        elif md is None:
            # on the copy stream: the rasteriser's hole-count read makes the host wait for the stream it runs on, and this one carries
            # input staging only (on the caller's stream the read waited behind whatever else the caller had queued there)
            if self.copy_stream is not None:
                with torch.cuda.stream(self.copy_stream):
                    md = _masks.random_masks(xd.shape[0], self.resolution, hole_range=self.hole_range, device=self.device,
                                             boxes=boxes).to(torch.float32)
                    md = md.reshape(xd.shape[0], 1, self.resolution, self.resolution)
                cur = torch.cuda.current_stream(self.device)
                cur.wait_stream(self.copy_stream)
                md.record_stream(cur)
            else:
                md = _masks.random_masks(xd.shape[0], self.resolution, hole_range=self.hole_range, device=self.device,
                                         boxes=boxes).to(torch.float32)
                md = md.reshape(xd.shape[0], 1, self.resolution, self.resolution)
        x4 = eval_harness.assemble_input(xd, md)
        return x4, xd, md, ids

    def __call__(self, loader):
        staged = None
        for batch in loader:
            nxt = self._stage(batch)              # copies of batch k+1 are in flight ...
            if staged is not None:
                yield self._finish(staged)        # ... while batch k is handed to the generator
            staged = nxt
        if staged is not None:
            yield self._finish(staged)


# ------------------------------------------------------------------------------------------------
# Places2 (lib/data_factory/ds_places2.py): images of their own sizes, resized to R x R on the device
# ------------------------------------------------------------------------------------------------

_PLACES2_TAGS = {
    # tagging_normal: under root_dir
    'train': ('data_large', '00train', ()), 'challenge': ('data_challenge', '01challenge', ()), 'val': ('val_large', '50val', ()),
    'test': ('test_large', '90test', ()),
    # tagging_small / tagging_small_512: under root_dir/places2_small
    'strain': ('train_large', '01strain', ('places2_small',)), 'sval': ('val_large', '51sval', ('places2_small',)),
    'stest': ('test_large', '91stest', ('places2_small',)),
    'strain512': ('train_512', '02strain', ('places2_small',)), 'sval512': ('val_512', '52val', ('places2_small',)),
    'stest512': ('test_512', '92test', ('places2_small',)),
    # tagging_fromtf
    'test_fromtf': ('test_fromtf/image', '93test_fromtf', ()),
}


def places2_list(root_dir, mode):
    """load_info of ``places2`` (ds_places2.py:19-77) in ds_base's order (sorted by unique_id, common/ds_base.py:50-51): every .jpg / .png
    under the mode's directory (``+``-joined modes concatenate), unique_id = '-'.join([maintag] + subdir.split('/')[4:] + [stem]) -- the
    reference's id, taken literally from the path string as given (its [4:] assumes a root four components deep)."""
    info = []
    for m in mode.split('+'):
        if m not in _PLACES2_TAGS:
            raise ValueError(m)
        imdir, maintag, mid = _PLACES2_TAGS[m]
        imdir = os.path.join(root_dir, *mid, imdir)
        for subdir, _, files in os.walk(imdir):
            for fi in files:
                impath = os.path.join(subdir, fi)
                if not (impath.endswith('.jpg') or impath.endswith('.png')):
                    continue
                uid = '-'.join([maintag] + subdir.split('/')[4:] + [os.path.splitext(fi)[0]])
                info.append({'unique_id': uid, 'filename': fi, 'image_path': impath})
    info = sorted(info, key=lambda x: x['unique_id'])
    for idx, e in enumerate(info):
        e['idx'] = idx
    return info


class Places2(torch.utils.data.Dataset):
    """``places2`` + ``FixResolutionLoader`` + ``FreeFormMaskFormatter`` (ds_places2.py:90-103,214-229) with the resize moved to the
    device: an item is {'image': uint8 [H,W,3] at the file's own size (``Image.open(...).convert('RGB')``, no EXIF rotation, as the
    reference), 'flip': the formatter's flip decision (one ``npr.rand()`` draw when ``random_flip``), 'unique_id'} and, with
    ``host_masks``, 'mask' = ``RandomMask(resolution, hole_range)[0]`` drawn after the flip, as the formatter does.  ``collate_ragged``
    batches items into a ``RaggedU8Batch``; ``DeviceFeeder`` resizes it (Pillow's bicubic bit for bit) and flips on the device.
    Without ``host_masks`` the masks come from the device (``DeviceFeeder(device_masks=True)``, the same numpy draws).

    ``mask_kind`` = 'lama_thin' | 'lama_medium' | 'lama_thick' (``LamaMaskFormatter``, the configs ``places2_val*_inpainting_lama{1,2,3}``):
    host masks are ``data.LamaMask(resolution, kind)[0]`` instead, drawn after the flip; on the device, ``DeviceFeeder(mask_kind=...)``.

    ``formatter='adv'`` is the training input, ``AdvInpaintingFormatter`` (ds_places2.py:183-207) behind the same loader: no flip; the
    item carries 'crop' = ``draw_scale_crop(R, R, R, flips=False)`` (the loader's output is R x R) and 'preresize', and the mask is
    drawn after those draws.  ``DeviceFeeder`` resizes to R x R as above and cuts the window of the float bicubic rescale on the device."""

    def __init__(self, root_dir, mode, resolution=512, random_flip=False, hole_range=(0, 1), host_masks=False, try_sample=None, repeat=1,
                 formatter='freeform', mask_kind='freeform'):
        if formatter not in ('freeform', 'adv'):
            raise ValueError(f"Places2: formatter must be 'freeform' or 'adv' (got {formatter!r})")
        self.mask_kind = _check_mask_kind('Places2', mask_kind)
        if mask_kind != 'freeform':
            if formatter != 'freeform':
                raise ValueError("Places2: LaMa masks go with formatter='freeform' (LamaMaskFormatter has no scale / crop draws)")
            LamaMaskFormatter(resolution=int(resolution), type=mask_kind[5:])        # ValueError outside the six settings
        self.load_info = places2_list(root_dir, mode)
        if try_sample is not None:
            self.load_info = self.load_info[:try_sample]
        self.resolution, self.random_flip, self.hole_range = int(resolution), bool(random_flip), list(hole_range)
        self.host_masks, self.repeat, self.formatter = bool(host_masks), repeat, formatter

    def __len__(self):
        return len(self.load_info) * self.repeat

    def __getitem__(self, idx):
        from PIL import Image
        e = self.load_info[idx % len(self.load_info)]
        with Image.open(e['image_path']) as im:
            u8 = np.asarray(im.convert('RGB'))
        if self.formatter == 'adv':
            item = {'image': u8, 'flip': False, 'unique_id': e['unique_id'], 'preresize': True,
                    'crop': draw_scale_crop(self.resolution, self.resolution, self.resolution, flips=False)}
        else:
            item = {'image': u8, 'flip': bool(self.random_flip and npr.rand() < 0.5), 'unique_id': e['unique_id']}
        if self.host_masks and self.mask_kind != 'freeform':
            item['mask'] = _data.LamaMask(self.resolution, self.mask_kind)[0]
        elif self.host_masks:
            item['mask'] = _data.RandomMask(self.resolution, self.hole_range)[0]
        return item


def places2_val256_inpainting(root_dir, **kw):
    """configs/dataset/places2.yaml ``places2_val256_inpainting``."""
    return Places2(root_dir, 'val', resolution=256, random_flip=False, hole_range=(0.0, 1.0), **kw)


def places2_val512_inpainting(root_dir, **kw):
    """configs/dataset/places2.yaml ``places2_val512_inpainting``."""
    return Places2(root_dir, 'val', resolution=512, random_flip=False, hole_range=(0.0, 1.0), **kw)


def _places2_lama(resolution, kind):
    def make(root_dir, **kw):
        return Places2(root_dir, 'val', resolution=resolution, random_flip=False, hole_range=(0.0, 1.0), mask_kind=kind, **kw)
    make.__doc__ = f"configs/dataset/places2.yaml: ``places2_val{resolution}_inpainting`` with ``LamaMaskFormatter(False, {resolution}, '{kind[5:]}')``."
    return make


# configs/dataset/places2.yaml ``places2_val{256,512}_inpainting_lama{1,2,3}``: 1 = thin, 2 = medium, 3 = thick
places2_val256_inpainting_lama1, places2_val256_inpainting_lama2, places2_val256_inpainting_lama3 = (
    _places2_lama(256, k) for k in ('lama_thin', 'lama_medium', 'lama_thick'))
places2_val512_inpainting_lama1, places2_val512_inpainting_lama2, places2_val512_inpainting_lama3 = (
    _places2_lama(512, k) for k in ('lama_thin', 'lama_medium', 'lama_thick'))


def places2_challenge256_inpainting(root_dir, **kw):
    """configs/dataset/places2.yaml ``places2_challenge256_inpainting``."""
    return Places2(root_dir, 'challenge', resolution=256, random_flip=True, hole_range=(0.0, 1.0), **kw)


def places2_challenge512_inpainting(root_dir, **kw):
    """configs/dataset/places2.yaml ``places2_challenge512_inpainting``."""
    return Places2(root_dir, 'challenge', resolution=512, random_flip=True, hole_range=(0.0, 1.0), **kw)


def places2_train256_adv_inpainting(root_dir, **kw):
    """Places2 training input at 256: ``FixResolutionLoader(256)`` + ``AdvInpaintingFormatter(256)`` (ds_places2.py:90-103,183-207)."""
    return Places2(root_dir, 'train', resolution=256, formatter='adv', hole_range=(0.0, 1.0), **kw)


def places2_train512_adv_inpainting(root_dir, **kw):
    """Places2 training input at 512: ``FixResolutionLoader(512)`` + ``AdvInpaintingFormatter(512)``."""
    return Places2(root_dir, 'train', resolution=512, formatter='adv', hole_range=(0.0, 1.0), **kw)


# ------------------------------------------------------------------------------------------------
# OpenImages (lib/data_factory/ds_openimages.py): images larger than R are resized to fit, then padded to R x R on the device
# ------------------------------------------------------------------------------------------------

_OPENIMAGES_DIRS = {'train': 'train', 'val': 'validation'}


def openimages_list(root_dir, mode):
    """load_info of ``openimages`` (ds_openimages.py:20-48) in ds_base's order (sorted by unique_id): every .jpg / .png under
    root_dir/train ('train') or root_dir/validation ('val'), unique_id = '-'.join(subdir.split('/')[4:] + [stem]) -- no main tag,
    unlike Places2; taken literally from the path string as given."""
    if mode not in _OPENIMAGES_DIRS:
        raise ValueError(mode)
    imdir = os.path.join(root_dir, _OPENIMAGES_DIRS[mode])
    info = []
    for subdir, _, files in os.walk(imdir):
        for fi in files:
            impath = os.path.join(subdir, fi)
            if not (impath.endswith('.jpg') or impath.endswith('.png')):
                continue
            uid = '-'.join(subdir.split('/')[4:] + [os.path.splitext(fi)[0]])
            info.append({'unique_id': uid, 'filename': fi, 'image_path': impath})
    info = sorted(info, key=lambda x: x['unique_id'])
    for idx, e in enumerate(info):
        e['idx'] = idx
    return info


def _decode_rgb_unbounded(path):
    """``Image.open(path).convert('RGB')`` with Pillow's decompression-bomb check off, as the reference's module sets
    ``PIL.Image.MAX_IMAGE_PIXELS = None`` -- here only for this decode: the process-wide limit is restored afterwards."""
    from PIL import Image
    old = Image.MAX_IMAGE_PIXELS
    Image.MAX_IMAGE_PIXELS = None
    try:
        with Image.open(path) as im:
            return np.asarray(im.convert('RGB'))
    finally:
        Image.MAX_IMAGE_PIXELS = old


def fill_outside_box(mask, content_size):
    """The box fill of OpenImages' FreeFormMaskFormatter (ds_openimages.py:161-163), in place on a [.., R, R] mask: keep (1) at every
    column >= w' and every row >= h'."""
    h, w = int(content_size[0]), int(content_size[1])
    mask[..., :, w:] = 1.0
    mask[..., h:, :] = 1.0
    return mask


class OpenImages(torch.utils.data.Dataset):
    """``openimages`` + ``FixResolutionLoader`` + ``FreeFormMaskFormatter`` (ds_openimages.py:63-81,148-166) with the resize and the
    padding moved to the device: an item is {'image': uint8 [H,W,3] at the file's own size (``Image.open(...).convert('RGB')``, no
    decompression-bomb limit), 'flip' (one ``npr.rand()`` draw when ``random_flip``), 'unique_id', 'content_size': (h', w') =
    ``resize.fit_size`` -- the box the image fills at the top-left of the R x R canvas} and, with ``host_masks``, 'mask' =
    ``RandomMask(resolution, hole_range)[0]`` drawn after the flip, then set to 1 at columns >= w' and rows >= h'.

    The reference's quirk is kept: the fill uses the UNFLIPPED box even when the flip has moved the content to the right edge, and
    RandomMask's hole-ratio test sees the whole mask, before the fill.  ``collate_ragged`` makes a ``RaggedU8Batch`` with ``fit`` set;
    ``DeviceFeeder`` resizes, pads and flips it on the device and, with device masks, applies the same fill there.

    ``formatter='adv'`` is the training input, ``AdvInpaintingFormatter`` (ds_openimages.py:117-141) behind the same loader: no flip,
    'crop' = ``draw_scale_crop(R, R, R, flips=False)`` of the padded R x R canvas, and -- as in the reference -- NO box fill: the mask is
    ``RandomMask`` as drawn, on the host and on the device alike."""

    def __init__(self, root_dir, mode, resolution=1024, random_flip=False, hole_range=(0, 1), host_masks=False, try_sample=None,
                 repeat=1, formatter='freeform'):
        if formatter not in ('freeform', 'adv'):
            raise ValueError(f"OpenImages: formatter must be 'freeform' or 'adv' (got {formatter!r})")
        self.formatter = formatter
        self.load_info = openimages_list(root_dir, mode)
        if try_sample is not None:
            self.load_info = self.load_info[:try_sample]
        self.resolution, self.random_flip, self.hole_range = int(resolution), bool(random_flip), list(hole_range)
        self.host_masks, self.repeat = bool(host_masks), repeat

    def __len__(self):
        return len(self.load_info) * self.repeat

    def __getitem__(self, idx):
        from .resize import fit_size
        e = self.load_info[idx % len(self.load_info)]
        u8 = _decode_rgb_unbounded(e['image_path'])
        try:
            box = fit_size(u8.shape[0], u8.shape[1], self.resolution)
        except ValueError as err:
            raise ValueError(f'{e["image_path"]}: {err}') from None
        if self.formatter == 'adv':
            item = {'image': u8, 'flip': False, 'unique_id': e['unique_id'], 'content_size': box, 'preresize': True,
                    'crop': draw_scale_crop(self.resolution, self.resolution, self.resolution, flips=False)}
            if self.host_masks:
                item['mask'] = _data.RandomMask(self.resolution, self.hole_range)[0]
            return item
        item = {'image': u8, 'flip': bool(self.random_flip and npr.rand() < 0.5), 'unique_id': e['unique_id'], 'content_size': box}
        if self.host_masks:
            item['mask'] = fill_outside_box(_data.RandomMask(self.resolution, self.hole_range)[0], box)
        return item


def openimages_val_1024(root_dir, **kw):
    """configs/dataset/openimages.yaml ``openimages_val_1024``."""
    return OpenImages(root_dir, 'val', resolution=1024, random_flip=False, hole_range=(0.0, 1.0), **kw)


def openimages_train_1024(root_dir, **kw):
    """configs/dataset/openimages.yaml ``openimages_train_1024``."""
    return OpenImages(root_dir, 'train', resolution=1024, random_flip=True, hole_range=(0.0, 1.0), **kw)


def openimages_train_1024_adv(root_dir, **kw):
    """OpenImages training input: ``FixResolutionLoader(1024)`` + ``AdvInpaintingFormatter(1024)`` (ds_openimages.py:63-81,117-141)."""
    return OpenImages(root_dir, 'train', resolution=1024, formatter='adv', hole_range=(0.0, 1.0), **kw)


# ------------------------------------------------------------------------------------------------
# random scale, random crop (the training formatters) and DTD (lib/data_factory/ds_texture.py)
# ------------------------------------------------------------------------------------------------

def draw_scale_crop(oh, ow, s, flips=False):
    """The draws of AdvInpaintingFormatter / InpaintingFormatter for an oh x ow image and window s, in the reference's order
    (ds_texture.py:138-147): nh, nw from ``npr.randint(s, max(o, int(s*1.2)) + 1)``, then ch, cw from ``npr.randint(0, n - s + 1)`` and,
    with ``flips`` (the texture formatter), two ``npr.random() < 0.5`` draws, vertical first -> (nh, nw, ch, cw, flip_v, flip_h) ints.
    The formatter draws its mask after these."""
    oh, ow, s = int(oh), int(ow), int(s)
    if s < 1 or oh < 1 or ow < 1:
        raise ValueError(f'draw_scale_crop: sizes must be >= 1 (got {oh}x{ow}, s = {s})')
    nh = npr.randint(s, max(oh, int(s * 1.2)) + 1)
    nw = npr.randint(s, max(ow, int(s * 1.2)) + 1)
    ch, cw = npr.randint(0, nh - s + 1), npr.randint(0, nw - s + 1)
    fv = fh = False
    if flips:
        fv = npr.random() < 0.5
        fh = npr.random() < 0.5
    return int(nh), int(nw), int(ch), int(cw), int(fv), int(fh)


def texture_list(root_dir, mode, mixed_order=False):
    """load_info of ``texture`` (ds_texture.py:25-89): the lines 'type/file' of root_dir/dtd/labels/<name>.txt for every ``+``-separated
    name in ``mode``, image at root_dir/dtd/images/<type>/<file>, unique_id = the file stem, in ds_base's order (sorted by unique_id).
    The reference's check of the mode names never raises (each name fails one of its three ``find(...) != 0`` tests), so any list name is
    accepted here too.  ``mixed_order`` (``mixed_order_on_texture_type``, :63-89): round-robin over the texture types in order of first
    appearance, each id prefixed with its position as '{:05d}_' -- the prefix is what makes ds_base's sort keep that order."""
    info = []
    for m in mode.split('+'):
        with open(os.path.join(root_dir, 'dtd', 'labels', m + '.txt')) as f:
            refs = [li.strip() for li in f.readlines()]
        for ref in refs:
            texture_type, filename = os.path.split(ref)
            info.append({'unique_id': os.path.splitext(filename)[0], 'filename': filename, 'texture_type': texture_type,
                         'image_path': os.path.join(root_dir, 'dtd', 'images', texture_type, filename)})
    if mixed_order:
        group = {}
        for e in info:
            group.setdefault(e['texture_type'], []).append(e)
        info, cnt = [], 0
        while group:
            for tt in list(group.keys()):
                if not group[tt]:
                    group.pop(tt)
                    continue
                e = dict(group[tt].pop(0))
                e['unique_id'] = '{:05d}_'.format(cnt) + e['unique_id']
                info.append(e)
                cnt += 1
    info = sorted(info, key=lambda x: x['unique_id'])
    for idx, e in enumerate(info):
        e['idx'] = idx
    return info


class Texture(torch.utils.data.Dataset):
    """``texture`` + ``DefaultLoader`` + ``InpaintingFormatter`` (ds_texture.py:22-100,121-149) with the rescale, crop and flips moved
    to the device: an item is {'image': uint8 [H,W,3] at the file's own size (``Image.open(...).convert('RGB')``), 'crop': the
    formatter's draws for that size (``draw_scale_crop(H, W, resolution, flips=True)``), 'flip': False, 'unique_id'} and, with
    ``host_masks``, 'mask' = ``RandomMask(resolution, hole_range)[0]`` drawn after them -- for the same numpy RNG state the reference
    formatter's parameters and mask.  ``collate_ragged`` batches items into a ``RaggedU8Batch`` with ``crop``; ``DeviceFeeder`` computes
    the windows on the device.  ``mode``: ``+``-separated list names under dtd/labels; the reference's mode check never raises, so any
    name is accepted (``texture_list``)."""

    def __init__(self, root_dir, mode, resolution, hole_range, mixed_order=False, host_masks=False, try_sample=None, repeat=1):
        self.load_info = texture_list(root_dir, mode, mixed_order=mixed_order)
        if try_sample is not None:
            self.load_info = self.load_info[:try_sample]
        self.resolution, self.hole_range = int(resolution), list(hole_range)
        self.host_masks, self.repeat = bool(host_masks), repeat

    def __len__(self):
        return len(self.load_info) * self.repeat

    def __getitem__(self, idx):
        e = self.load_info[idx % len(self.load_info)]
        u8 = _decode_rgb_unbounded(e['image_path'])           # ds_texture.py:12 lifts Pillow's pixel limit as ds_openimages.py does
        item = {'image': u8, 'flip': False, 'unique_id': e['unique_id'],
                'crop': draw_scale_crop(u8.shape[0], u8.shape[1], self.resolution, flips=True)}
        if self.host_masks:
            item['mask'] = _data.RandomMask(self.resolution, self.hole_range)[0]
        return item


def texture_train_256(root_dir, **kw):
    """DTD training input at 256: ``texture`` (lists train1 + val1) + ``InpaintingFormatter(256)``."""
    return Texture(root_dir, 'train1+val1', resolution=256, hole_range=(0.0, 1.0), **kw)


def texture_train_512(root_dir, **kw):
    """DTD training input at 512: ``texture`` (lists train1 + val1) + ``InpaintingFormatter(512)``."""
    return Texture(root_dir, 'train1+val1', resolution=512, hole_range=(0.0, 1.0), **kw)


class RaggedU8Batch:
    """A batch of decoded images of their own sizes: ``data`` uint8 [sum h*w*3] (HWC RGB images back to back, pinned when built in a
    process that owns the device), ``shapes`` int32 [B,3] = (h, w, byte offset), ``flip`` bool [B], ``ids``, ``masks`` float32 [B,R,R] or
    None.  ``DeviceFeeder`` / ``EvalLoop.run`` take it in place of an image tensor; ``pin_memory`` lets a DataLoader pin it.
    ``fit`` (OpenImages): the images are resized to ``content_size`` int32 [B,2] = (h', w') and padded to R x R instead of resized to
    R x R (Places2: ``fit`` False, ``content_size`` None).
    ``crop`` (the training formatters): int32 [B,6] = (nh, nw, ch, cw, flip_v, flip_h) of ``draw_scale_crop`` or None; with it the batch
    becomes float32 windows on the device, cut from the images themselves or, when ``preresize``, from the loader's R x R resize."""

    def __init__(self, data, shapes, flip, ids, masks=None, fit=False, content_size=None, crop=None, preresize=False):
        self.data, self.shapes, self.flip, self.ids, self.masks = data, shapes, flip, list(ids), masks
        self.fit, self.content_size = bool(fit), content_size
        self.crop, self.preresize = crop, bool(preresize)

    def __len__(self):
        return int(self.shapes.shape[0])

    def pin_memory(self):
        if not self.data.is_pinned():
            self.data = self.data.pin_memory()
        return self


def collate_ragged(items):
    """Places2, OpenImages or Texture items -> RaggedU8Batch (``torch.utils.data.DataLoader(collate_fn=collate_ragged)``); items with a
    'content_size' (OpenImages) make a ``fit`` batch, items with a 'crop' (the training formatters) a batch with ``crop``."""
    from .resize import pack_images
    data, shapes = pack_images([it['image'] for it in items])
    flip = torch.tensor([bool(it['flip']) for it in items], dtype=torch.bool)
    masks = None
    if all('mask' in it for it in items) and items:
        masks = torch.from_numpy(np.stack([np.asarray(it['mask'], np.float32) for it in items]))
    if torch.utils.data.get_worker_info() is None and torch.cuda.is_available():
        data = data.pin_memory()
    fit = bool(items) and all('content_size' in it for it in items)
    if not fit and any('content_size' in it for it in items):
        raise ValueError('collate_ragged: a batch mixes OpenImages items (content_size) with items resized to R x R')
    content_size = torch.tensor([list(it['content_size']) for it in items], dtype=torch.int32).reshape(-1, 2) if fit else None
    crop = None
    if any('crop' in it for it in items):
        if not all('crop' in it for it in items) or len({bool(it.get('preresize', False)) for it in items}) != 1:
            raise ValueError('collate_ragged: a batch mixes items of different formatters (crop / preresize)')
        crop = torch.tensor([list(it['crop']) for it in items], dtype=torch.int32).reshape(-1, 6)
    return RaggedU8Batch(data, shapes, flip, [it['unique_id'] for it in items], masks, fit=fit, content_size=content_size, crop=crop,
                         preresize=crop is not None and bool(items[0].get('preresize', False)))
