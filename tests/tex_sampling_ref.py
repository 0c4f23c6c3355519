"""Texture sampling records in numpy float32, restated from the text of INTEGRATION.md "Texture sampling" (not from the C code): the coordinate transform and
the wrap modes, the nearest and the bilinear lookup of a colour texture, the bilinear lookup of a normal map, and the lookup without records that an identity
record (and no record) selects.  Every operation is one float32 operation in the order of the text."""
import numpy as np

f32 = np.float32
CLAMP, REPEAT, MIRROR = 0, 1, 2
DEFAULT, NEAREST, BILINEAR = 0, 1, 2
S255 = f32(1.0) / f32(255.0)


class Sampler:
    def __init__(self, wrap_u=CLAMP, wrap_v=None, filter=DEFAULT, scale=(1.0, 1.0), offset=(0.0, 0.0)):
        self.wrap_u = wrap_u; self.wrap_v = wrap_u if wrap_v is None else wrap_v; self.filter = filter
        self.scale = (f32(scale[0]), f32(scale[1])); self.offset = (f32(offset[0]), f32(offset[1]))

    def identity(self, normal_map=False):
        own = BILINEAR if normal_map else NEAREST
        return (self.wrap_u == CLAMP and self.wrap_v == CLAMP and self.filter in (DEFAULT, own) and self.scale == (f32(1), f32(1))
                and self.offset == (f32(0), f32(0)))


def coord(c, scale, offset, wrap):
    """t = c * scale + offset; not finite: 0; else the wrap mode"""
    with np.errstate(all="ignore"):
        c = np.asarray(c, f32)
        t = ((c * f32(scale)).astype(f32) + f32(offset)).astype(f32)
        fin = np.isfinite(t)
        t = np.where(fin, t, f32(0)).astype(f32)
        if wrap == CLAMP:
            r = np.where(t < 0, f32(0), np.where(t > 1, f32(1), t))
        elif wrap == REPEAT:
            r = (t - np.floor(t)).astype(f32)
        else:
            k = np.floor(t).astype(f32); f = (t - k).astype(f32)
            odd = (k - (f32(2) * np.floor((k * f32(0.5)).astype(f32)).astype(f32)).astype(f32)).astype(f32) == 1
            r = np.where(odd, (f32(1) - f).astype(f32), f)
        return np.where(fin, r, f32(0)).astype(f32)


def _uv(s, uv):
    uv = np.asarray(uv, f32).reshape(-1, 2)
    u = coord(uv[:, 0], s.scale[0], s.offset[0], s.wrap_u)
    v = (f32(1) - coord(uv[:, 1], s.scale[1], s.offset[1], s.wrap_v)).astype(f32)        # the flip, after wrapping
    return u, v


def _index(i, size, wrap):
    return np.mod(i, size) if wrap == REPEAT else np.clip(i, 0, size - 1)


def _taps(s, w, h, u, v):
    x = ((u * f32(w)).astype(f32) - f32(0.5)).astype(f32); y = ((v * f32(h)).astype(f32) - f32(0.5)).astype(f32)
    x0 = np.floor(x).astype(f32); y0 = np.floor(y).astype(f32)
    fx = (x - x0).astype(f32); fy = (y - y0).astype(f32)
    i0 = x0.astype(np.int64); j0 = y0.astype(np.int64)
    return (_index(i0, w, s.wrap_u), _index(i0 + 1, w, s.wrap_u), _index(j0, h, s.wrap_v), _index(j0 + 1, h, s.wrap_v), fx, fy)


def _lerp(a, b, c, d, fx, fy):
    r0 = (a + (fx * (b - a).astype(f32)).astype(f32)).astype(f32); r1 = (c + (fx * (d - c).astype(f32)).astype(f32)).astype(f32)
    return (r0 + (fy * (r1 - r0).astype(f32)).astype(f32)).astype(f32)


def nearest_clamp(img, uv):
    """the lookup without records (FImageTexture::Sample): clamp, flip, nearest; a NaN coordinate selects texel 0 on its axis -> (n, 3) uint8"""
    img = np.asarray(img, np.uint8); h, w, _ = img.shape
    uv = np.asarray(uv, f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        u = np.where(uv[:, 0] < 0, f32(0), np.where(uv[:, 0] > 1, f32(1), uv[:, 0])).astype(f32)
        v = (f32(1) - np.where(uv[:, 1] < 0, f32(0), np.where(uv[:, 1] > 1, f32(1), uv[:, 1])).astype(f32)).astype(f32)
        fi = (u * f32(w)).astype(f32); fj = (v * f32(h)).astype(f32)
        i = np.where(fi >= 0, fi, f32(0)).astype(np.int64); j = np.where(fj >= 0, fj, f32(0)).astype(np.int64)
    return img[np.minimum(j, h - 1), np.minimum(i, w - 1)]


def lookup(s, img, uv):
    """a colour texture under the record s (None or the identity: nearest_clamp) -> (n, 3) uint8"""
    img = np.asarray(img, np.uint8); h, w, _ = img.shape
    if s is None or s.identity():
        return nearest_clamp(img, uv)
    u, v = _uv(s, uv)
    if s.filter != BILINEAR:
        i = np.minimum((u * f32(w)).astype(f32).astype(np.int64), w - 1); j = np.minimum((v * f32(h)).astype(f32).astype(np.int64), h - 1)
        return img[j, i]
    i0, i1, j0, j1, fx, fy = _taps(s, w, h, u, v)
    F = img.astype(f32)
    r = _lerp(F[j0, i0], F[j0, i1], F[j1, i0], F[j1, i1], fx[:, None], fy[:, None])
    return np.minimum((r + f32(0.5)).astype(f32).astype(np.int64), 255).astype(np.uint8)


def color(s, img, uv):
    """the albedo of the lookup: (1 / 255) * byte"""
    return (S255 * lookup(s, img, uv).astype(f32)).astype(f32)


def nmap_decode(b):
    return np.maximum(((b.astype(f32) - f32(128)) / f32(127)).astype(f32), f32(-1))


def nmap_lookup(s, img, uv):
    """the tangent-space vector of a normal map under an ACTIVE record s (bilinear between decoded texels) -> (n, 3) float32"""
    img = np.asarray(img, np.uint8); h, w, _ = img.shape
    u, v = _uv(s, uv)
    i0, i1, j0, j1, fx, fy = _taps(s, w, h, u, v)
    D = nmap_decode(img)
    return _lerp(D[j0, i0], D[j0, i1], D[j1, i0], D[j1, i1], fx[:, None], fy[:, None])
