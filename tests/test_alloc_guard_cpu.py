"""tests/alloc_guard.py on CPU tensors (no GPU): every replaced factory and dtype family, what the housed tensor keeps, the poison, the
records of a damaged guard, what passes through, what is restored, and the refusal to nest with tests/alloc_fill.py."""
import numpy as np
import pytest
import torch

import alloc_fill
import alloc_guard
from alloc_fill import filled
from alloc_guard import guarded

BAND = 1024          # (any multiple of 512; small keeps these tests quick)
FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.complex64)
BYTES = (torch.uint8, torch.int8)
WIDE = (torch.int16, torch.int32, torch.int64)


def _raw(a):
    return a.raw.numpy()


def _same_layout(g, p):
    assert (g.shape, g.stride(), g.dtype, g.device, g.requires_grad, g.is_pinned()) == (p.shape, p.stride(), p.dtype, p.device, p.requires_grad, p.is_pinned())
    assert g.is_contiguous() == p.is_contiguous()
    if g.dim() == 4:
        assert g.is_contiguous(memory_format=torch.channels_last) == p.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize('dtype', FLOATS + BYTES + WIDE + (torch.bool,))
def test_layout_of_the_raw_buffer_and_the_poison_per_dtype(dtype):
    with guarded(band=BAND) as rec:
        t = torch.empty(3, 5, dtype=dtype)
        a = rec.allocations[0]
        nbytes = 15 * t.element_size()
        raw = _raw(a)
        assert rec.count == 1 and a.nbytes == nbytes and raw.size == 2 * BAND + nbytes and (a.shape, a.dtype, a.factory) == ((3, 5), dtype, 'empty')
        assert t.data_ptr() == a.raw.data_ptr() + BAND and not raw[BAND:BAND + nbytes].any()           # zero interior, right behind the front guard
        front, back = raw[:BAND], raw[BAND + nbytes:]                                                   # the back guard starts at the first byte after it
        if dtype in WIDE:
            assert (front.view(t.numpy().dtype) == 3).all() and (back.view(t.numpy().dtype) == 3).all()
        elif dtype == torch.bool:
            assert (front == 1).all() and (back == 1).all()
        else:
            assert (front == 0xFF).all() and (back == 0xFF).all()
            if dtype.is_floating_point:
                assert bool(torch.isnan(a.raw[:BAND].view(dtype)).all())
        assert rec.violations() == []


def test_every_factory_keeps_what_the_original_returns():
    src = torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    perm = torch.zeros(2, 3, 4, dtype=torch.float64).permute(2, 0, 1)
    calls = {
        'empty': lambda: torch.empty((2, 8, 3, 5), dtype=torch.float16, memory_format=torch.channels_last),
        'empty_like': lambda: torch.empty_like(src),
        'empty_like_permuted': lambda: torch.empty_like(perm),
        'empty_like_half': lambda: torch.empty_like(src, dtype=torch.float16),
        'new_empty': lambda: src.new_empty((2, 2), dtype=torch.int32),
        'zeros': lambda: torch.zeros(3, 4),
        'zeros_grad': lambda: torch.zeros([5], requires_grad=True),
        'ones': lambda: torch.ones([2, 2], dtype=torch.float64),
        'full': lambda: torch.full((3,), 7, dtype=torch.int64),
        'full_scalar': lambda: torch.full([], 2.5),
        'zeros_like': lambda: torch.zeros_like(perm),
        'ones_like': lambda: torch.ones_like(src, dtype=torch.bool),
        'full_like': lambda: torch.full_like(src, float('inf')),
        'new_zeros': lambda: src.new_zeros((4,)),
        'new_ones': lambda: src.new_ones((2, 3), dtype=torch.uint8),
        'new_full': lambda: src.new_full((2,), -1.5),
    }
    plain = {k: c() for k, c in calls.items()}
    with torch.enable_grad(), guarded(band=BAND) as rec:
        housed = {k: c() for k, c in calls.items()}
        assert rec.count == len(calls) and [a.factory for a in rec.allocations] == [max((f for f in alloc_guard.FACTORIES if k.startswith(f)), key=len)
                                                                                  for k in calls]
        assert rec.violations() == []
    for k, g in housed.items():
        _same_layout(g, plain[k])
        if k.startswith(('empty', 'new_empty')):
            assert not bool(g.any()), k                       # the interior is zero
        else:
            assert torch.equal(g, plain[k]), k                # an initialising factory writes its own value
    assert housed['empty_like_permuted'].stride() == perm.stride() and housed['zeros_grad'].is_leaf


def test_zero_size_meta_and_out_calls():
    with guarded(band=BAND) as rec:
        a = torch.empty((0, 1, 32, 32))
        b = torch.zeros(0, dtype=torch.int32)
        c = torch.empty_like(a)
        assert rec.count == 3 and a.numel() == b.numel() == c.numel() == 0 and tuple(a.shape) == (0, 1, 32, 32) and rec.violations() == []
        m = torch.empty(4, device='meta')
        assert m.is_meta and rec.count == 3 and torch.zeros_like(m).is_meta and rec.count == 3          # meta tensors pass through
        out = torch.arange(4.0)
        assert torch.zeros(4, out=out) is out and rec.count == 3                                        # so does a call that is given its buffer


def test_to_on_the_host_passes_through():
    x = torch.arange(6.0)
    with guarded(band=BAND, operands=True) as rec:
        assert 'to' in vars(torch.Tensor) and 'cuda' in vars(torch.Tensor)
        assert x.to(torch.float32) is x and x.to('cpu') is x
        h = x.to(torch.float16)
        assert h.dtype == torch.float16 and torch.equal(h.float(), x) and rec.count == 0
        with torch.enable_grad():
            p = torch.nn.Parameter(x.clone())
            assert p.to(torch.float64).grad_fn is not None and rec.count == 0
    with guarded(band=BAND, operands=False):
        assert 'to' not in vars(torch.Tensor) and 'cuda' not in vars(torch.Tensor)


def test_a_damaged_guard_is_reported_with_side_size_offset_and_values():
    with guarded(band=BAND) as rec:
        y = torch.empty(2, 3)
        k = torch.empty(5, dtype=torch.int32)
        torch.empty(4, dtype=torch.float16)                                         # (stays whole)
        flat = y.as_strided((2 * BAND // 4 + 6,), (1,), 0)
        flat[BAND // 4 + 6 + 2] = 5.0                                               # the third float after the end
        flat[BAND // 4 + 6 + 3] = 6.0
        flat[0] = 1.0                                                               # the first float of the front guard
        ints = k.as_strided((2 * BAND // 4 + 5,), (1,), 0)
        ints[BAND // 4 - 1] = 3                                                     # the poison value itself: not seen
        ints[BAND // 4 - 2] = 259                                                   # 0x103: one byte differs from the poison
        found = rec.violations()
    assert [(v.side, v.shape, v.dtype, v.factory, v.site) for v in found] == [('front', (2, 3), torch.float32, 'empty', None), ('back', (2, 3), torch.float32, 'empty', None),
                                                                              ('front', (5,), torch.int32, 'empty', None)]
    front, back, wide = found
    assert (back.bytes, back.first_byte, back.last_byte, back.first_element, back.last_element) == (8, 8, 15, 2, 3) and back.values[:2] == [5.0, 6.0]
    assert (front.bytes, front.first_byte, front.last_byte, front.first_element, front.last_element) == (4, -BAND, -BAND + 3, -BAND // 4, -BAND // 4)
    assert front.values[0] == 1.0 and np.isnan(front.values[1])
    assert (wide.bytes, wide.first_byte, wide.last_byte, wide.first_element, wide.last_element) == (1, -7, -7, -2, -2) and wide.values == [259, 3]
    assert 'side back, 8 bytes at offset 8 .. 15 (elements 2 .. 3), found [5.0, 6.0' in repr(back)
    with pytest.raises(RuntimeError, match='inside'):
        rec.violations()                                                            # the raw buffers are released when the context ends


def test_the_buffers_live_until_the_context_ends():
    with guarded(band=BAND) as rec:
        ptrs = set()
        for _ in range(50):
            ptrs.add(torch.empty(16).data_ptr())                                    # dropped at once, yet no block is handed out twice
        assert len(ptrs) == 50 and rec.count == 50
    assert rec.closed and all(a.raw is None for a in rec.allocations)


def _patched():
    names = alloc_guard._FUNCTIONS
    methods = alloc_guard._METHODS + alloc_guard.OPERANDS
    return tuple(getattr(torch, n) for n in names) + tuple(getattr(torch.Tensor, n) for n in methods) + tuple(n in vars(torch.Tensor) for n in methods)


def test_everything_is_restored_after_an_exception():
    before = _patched()
    with pytest.raises(ZeroDivisionError):
        with guarded(band=BAND):
            now = _patched()
            n = len(alloc_guard._FUNCTIONS) + len(alloc_guard._METHODS) + len(alloc_guard.OPERANDS)
            assert all(a is not b for a, b in zip(now[:n], before[:n])) and all(now[n:])
            1 / 0
    assert _patched() == before and alloc_fill._active[0] is None
    with guarded(band=BAND):                                                        # and the helper is usable again
        pass
    assert _patched() == before


def test_no_nesting_with_itself_or_with_the_fill_in_either_direction():
    before = _patched()
    with guarded(band=BAND) as rec:
        with pytest.raises(RuntimeError, match='re-entrant'):
            with guarded(band=BAND):
                pass
        with pytest.raises(RuntimeError, match="re-entrant: 'guarded' is active"):
            with filled('nan'):
                pass
        torch.empty(3)
        assert rec.count == 1                                                       # the outer guard is still active
    with filled('nan'):
        with pytest.raises(RuntimeError, match="does not nest with alloc_fill.filled: 'nan' is active"):
            with guarded(band=BAND):
                pass
        assert bool(torch.isnan(torch.empty(3)).all())                              # the outer fill is still active
    assert _patched() == before and alloc_fill._active[0] is None


def test_the_band_is_a_multiple_of_512():
    for band in (0, 100, 513, -512):
        with pytest.raises(ValueError):
            with guarded(band=band):
                pass


def test_recorded_site_is_the_innermost_package_frame():
    import shgan_amd  # noqa: F401
    from shgan_amd import kernels, resize
    img = np.full((2, 3, 3), 7, np.uint8)
    with guarded(band=BAND) as rec:
        packed, shapes = resize.pack_images([img, img])
        torch.zeros(3)                                                              # from the test itself: no frame inside the package
        assert rec.sites == {('resize.py', 'pack_images')} and rec.count == 2 and rec.sites_of(alloc_guard.INITIALISING) == set()
        assert bool((packed == 7).all()) and shapes.tolist() == [[2, 3, 0], [2, 3, 18]] and rec.violations() == []
    with guarded(band=BAND) as rec:                                                 # the pass-through allocators are looked through
        t = kernels._Launch().new((2, 2))
        assert rec.count == 1 and rec.sites == set() and tuple(t.shape) == (2, 2)
