"""Recording stand-in for ``cv2`` (tools/gen_golden_lama.py puts this directory on ``sys.path``): the reference's LaMa mask generator
draws with ``cv2.line`` only; every call is recorded as plain integers and nothing is painted."""
calls = []


def line(img, pt1, pt2, color, thickness=1, *args, **kw):
    if args or kw or float(color) != 1.0:
        raise NotImplementedError('cv2 stand-in: line() with options the LaMa generator never passes')
    for v in (*pt1, *pt2, thickness):
        if int(v) != v:
            raise TypeError(f'cv2 stand-in: non-integer argument {v!r}')
    calls.append((int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1]), int(thickness), type(pt2[0]).__name__))
    return img


def circle(*args, **kw):
    raise NotImplementedError('cv2 stand-in: circle() is never called by the shipped LaMa settings')
