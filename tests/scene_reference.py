"""Float64 / numpy restatement of whole-scene tiling (change3d_amd/infer.py, csrc/scene_ops.hip), written independently of
both: the geometry, the reflect fold (checked against `np.pad(mode="reflect")` itself in test_scene_cpu.py), the window and
the stitch.  The stitch is a SCATTER: every tile is added into a padded float64 canvas and the canvas is divided -- the
product is a gather with a fixed tap order -- so the two share nothing but the definition sum(w * p) / sum(w)."""
import numpy as np

U = 2.0 ** -24       # unit roundoff of f32


def plan(extent, t, s):
    """(m, n, k, starts) of one axis; ValueError where the geometry is refused."""
    if not 1 <= s <= t:
        raise ValueError("1 <= s <= t")
    if (t - s) % 2:
        raise ValueError("t - s must be even")
    m = (t - s) // 2
    n = (extent + s - 1) // s
    k = (t + s - 1) // s
    return m, n, k, [i * s - m for i in range(n)]


def fold(c, extent):
    """One coordinate folded into [0, extent) the way np.pad(mode='reflect') lays a signal out: ... 2 1 0 1 2 ... E-1 E-2 ..."""
    if extent == 1:
        return 0
    period = 2 * (extent - 1)
    c = c % period                      # Python's %: non-negative
    return period - c if c >= extent else c


def window(name, t):
    if name == "flat":
        return np.ones(t, dtype=np.float32)
    i = np.arange(t, dtype=np.float64)
    return (np.sin(np.pi * (i + 0.5) / t) ** 2).astype(np.float32)


def padded(scene, th, tw, sy, sx):
    """The scene padded by np.pad(reflect) so that tile (i, j) is out[i*sy : i*sy + th, j*sx : j*sx + tw]."""
    Hs, Ws = scene.shape[:2]
    my, ny, _, _ = plan(Hs, th, sy)
    mx, nx, _, _ = plan(Ws, tw, sx)
    bottom, right = (ny - 1) * sy - my + th - Hs, (nx - 1) * sx - mx + tw - Ws
    return np.pad(scene, ((my, bottom), (mx, right)) + ((0, 0),) * (scene.ndim - 2), mode="reflect"), ny, nx


def crops(scene, th, tw, sy, sx):
    """uint8 [ny * nx, th, tw, 6] in row-major tile order, cut from the np.pad(reflect) image."""
    big, ny, nx = padded(scene, th, tw, sy, sx)
    return np.stack([big[i * sy:i * sy + th, j * sx:j * sx + tw] for i in range(ny) for j in range(nx)])


def stitch(tiles, Hs, Ws, sy, sx, wy, wx, drop_tap=None, transpose_window=False):
    """tiles [ny, nx, C, th, tw] -> dict(blend f64 [C, Hs, Ws], absw = sum(w |p|) / sum(w) [C, Hs, Ws], taps int [Hs, Ws]).
    drop_tap = (i, j) leaves that tile out; transpose_window uses w[x][y] in place of w[y][x] (negative controls)."""
    ny, nx, C, th, tw = tiles.shape
    my, mx = (th - sy) // 2, (tw - sx) // 2
    w = np.outer(wy.astype(np.float64), wx.astype(np.float64))
    if transpose_window:
        assert th == tw
        w = w.T.copy()
    Hc, Wc = (ny - 1) * sy + th, (nx - 1) * sx + tw
    num, absn = np.zeros((C, Hc, Wc)), np.zeros((C, Hc, Wc))
    den, taps = np.zeros((Hc, Wc)), np.zeros((Hc, Wc), dtype=np.int64)
    for i in range(ny):
        for j in range(nx):
            if drop_tap == (i, j):
                continue
            ys, xs = slice(i * sy, i * sy + th), slice(j * sx, j * sx + tw)
            p = tiles[i, j].astype(np.float64)
            num[:, ys, xs] += w * p
            absn[:, ys, xs] += w * np.abs(p)
            den[ys, xs] += w
            taps[ys, xs] += 1
    cut = (slice(my, my + Hs), slice(mx, mx + Ws))
    den = den[cut]
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(blend=num[(slice(None),) + cut] / den, absw=absn[(slice(None),) + cut] / den, taps=taps[cut])


def bound(ref):
    """Per-element bound on |f32 gather-form stitch - float64 blend|: (taps + 3) * 2^-24 * sum(w |p|) / sum(w).  See
    test_scene_ops_gpu.py for where the count comes from."""
    return (ref["taps"][None] + 3) * U * ref["absw"]
