"""The two colour maps the pictures use, `summer` and `gist_rainbow`, as 256-entry fp64 tables built here from their segment
definitions the way matplotlib builds its lookup tables; matplotlib is not needed at run time.  Lookup is matplotlib's: index
`int(x * 256)` (in the dtype of x) clipped to 0..255, a NaN gives (0, 0, 0)."""
import functools

import numpy as np

N = 256

# (x, (r, g, b)) control points, linear in between
_SUMMER = ((0.0, (0.0, 0.5, 0.4)), (1.0, (1.0, 1.0, 0.4)))
_GIST_RAINBOW = ((0.000, (1.00, 0.00, 0.16)), (0.030, (1.00, 0.00, 0.00)), (0.215, (1.00, 1.00, 0.00)), (0.400, (0.00, 1.00, 0.00)),
                 (0.586, (0.00, 1.00, 1.00)), (0.770, (0.00, 0.00, 1.00)), (0.954, (1.00, 0.00, 1.00)), (1.000, (1.00, 0.00, 0.75)))


def _channel(x, y):
    """one channel's table from control points without jumps: entry i is the interpolation at i / 255 scaled to index units"""
    x = np.asarray(x, np.float64) * (N - 1)
    y = np.asarray(y, np.float64)
    xind = (N - 1) * np.linspace(0, 1, N)
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y[0]], distance * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
    return np.clip(lut, 0.0, 1.0)


def _table(points):
    x = [p[0] for p in points]
    return np.stack([_channel(x, [p[1][c] for p in points]) for c in range(3)], axis=-1)


@functools.lru_cache(maxsize=None)
def summer_table():
    """fp64 [256, 3]: (i / 255, 0.5 + 0.5 * i / 255, 0.4)"""
    t = _table(_SUMMER)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def gist_rainbow_table():
    """fp64 [256, 3]"""
    t = _table(_GIST_RAINBOW)
    t.setflags(write=False)
    return t


def lookup(table, x):
    """numpy: table[int(x * 256) clipped to 0..255], fp64 [..., 3]; NaN -> (0, 0, 0).  x keeps its float dtype for the product."""
    x = np.asarray(x)
    if x.dtype.kind != "f":
        x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        xa = x * x.dtype.type(N)
        bad = np.isnan(xa)
        idx = np.where(xa >= N, N - 1, np.where(xa < 0, 0, np.where(bad, 0, xa))).astype(np.int64)
    out = table[idx]
    out[bad] = 0.0
    return out


def summer(x):
    return lookup(summer_table(), x)


def gist_rainbow(x):
    return lookup(gist_rainbow_table(), x)


_DEVICE_TABLES = {}


def device_table(name, device):
    """the fp64 [256, 3] table `name` ("summer" / "gist_rainbow") on `device`, uploaded once per device"""
    import torch

    key = (name, str(device))
    if key not in _DEVICE_TABLES:
        t = {"summer": summer_table, "gist_rainbow": gist_rainbow_table}[name]()
        _DEVICE_TABLES[key] = torch.from_numpy(t.copy()).to(device)
    return _DEVICE_TABLES[key]
