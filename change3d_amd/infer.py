"""Whole-scene change maps: a trained model, a pair of co-registered images of any size, a change map back.

The encoder's perception frames fix the model's input at `in_height x in_width`, so a scene is cut into overlapping tiles
of that size, every tile runs through the folded-BatchNorm eval forward, and the per-tile outputs are blended back with a
window.  The reference stops at `val()` over pre-cut crops (reference scripts/train_BCD.py:92-154, scripts/train_SCD.py:
104-178); nothing there tiles a scene.  Here the scene is uploaded once as uint8 `[Hs, Ws, 6]` and stays in HBM:
`c3d_scene_gather` cuts and normalises `batch` tiles per launch, `Trainer.update_bcd / update_scd` predicts them, and
`c3d_scene_stitch` writes each strip of scene rows as soon as the tile rows that cover it exist, from a ring of
`k = ceil(t / s)` tile rows.

Geometry, per axis, for tile `t` and stride `s` (`1 <= s <= t`, `t - s` even): margin `m = (t - s) / 2`,
`n = ceil(extent / s)` tiles, tile `i` starts at `i*s - m`.  Every scene pixel then lies in the central `s`-wide region of
some tile.  Coordinates outside the scene fold back as `np.pad(mode="reflect")` does, for any overhang.

BDA (xBD) is the third scene task: `update_bda`'s localisation head is stitched like the BCD probability (blend, mask =
blend > 0.5) and its damage head like an SCD class map (blended logits, argmax gated by the localisation mask).

`predict(scene, objects=True)` appends the objects of the map (`SceneObjects`): `c3d_scene_objects` labels the connected
components of the mask on the device, drops those below `min_area`, numbers the rest in raster order and fills one table
row per object -- area, box, mean probability, and the majority class of the class map inside it, which for BDA is the xBD
convention of one damage class per building.  It is enqueued behind the last strip: still one upload and one host
synchronisation per scene, nothing is read back.

`predict(scene, objects=True, outlines=True)` appends the polygons of those objects (`SceneOutlines`) after them:
`c3d_scene_outlines` traces the label map into closed rings on the device, one outline per object and one ring per hole, as
a ring table and a vertex list; it is enqueued behind the labelling, before the same one synchronisation.

`predict(scene, objects=True, outlines=True, simplify=tol)` appends one more `SceneOutlines` after the raw one: the same rings
simplified by `c3d_outlines_simplify` (Douglas-Peucker, `tol` in pixels), enqueued behind the tracing, before the same one
synchronisation.  Its rows are `(id, start, n_vertices, 2 * area, perimeter, x, y, raw n_vertices)`.

`predict(..., simplify=tol, simplify_shared=True)` puts a `SceneSharedOutlines` in that place instead: the rings cut at the points
where three or more regions of the label map meet and simplified once per arc between two such nodes
(`c3d_outlines_simplify_shared`), so that two neighbours -- the pieces of `split=R` above all -- share their wall vertex for
vertex.  Its first three fields are those of the simplified `SceneOutlines`, and every later stage takes it unchanged; `left` is
the label on the other side of the edge leaving each vertex, `info` counts nodes, arcs and collapsed rings.  Still the same one
synchronisation.

`predict(..., simplify=tol, simplify_shared=True, simplify_safe=True)` puts a `SceneSafeOutlines` there: the same call in rounds
(`c3d_outlines_simplify_safe`), in which every arc that takes part in a defect of the output -- chords that cross or overlap, a
vertex inside another edge, a ring that collapsed or flipped -- gets a smaller tolerance of its own until a round finds nothing
or `safe_rounds` rounds have run.  It is a `SceneSharedOutlines` with `.level`, the level of the arc of the edge leaving each
vertex, and `.safe` i64 [8], whose last element says whether the loop converged.  The rounds are launched ahead: still the same
one synchronisation.

`predict(..., simplify=tol, simplify_check=True)` appends a `SceneFill` after that: the simplified rings filled back into a
label map of the scene's size (`c3d_rings_fill`, centre sampling, even-odd per id) and joined to the raw objects with
`c3d_objects_match` at the lowest threshold, 0.5 -- per object what the simplification cost: its partner, intersection and union
in pixels.  Enqueued behind the simplification, before the same one synchronisation.

`predict(..., outlines=True, shapes=True)` appends a `SceneShapes` last: the convex hull and the minimum-area rectangle of
every object (`c3d_rings_hull`, integer rule of include/change3d_hip.h), taken from the raw rings whatever else was asked
for, enqueued before the same one synchronisation.

`predict(..., outlines=True, simplify=tol, regularize=True)` appends a `SceneRegular` after those: the simplified rings with
every edge parallel or perpendicular to the chosen rectangle edge of their object (`c3d_rings_regularize` on the hulls of the
raw rings; the hull call is shared with `shapes=True`), in sixteenths of a pixel.  `regularize_check=True` appends a `SceneFill`
of those rings after it, as `simplify_check` does for the simplified ones.  Still the same one synchronisation.

`predict(..., outlines=True, validity=True)` appends one `SceneValidity` per stage the call has, after everything above so that
no position moves: of the raw rings, then of the simplified ones with `simplify=tol`, then of the regularised ones (at 1/16 px)
with `regularize=True`.  `c3d_rings_valid` counts the proper crossings, collinear overlaps and touches among the edges of every
object, holes included; an object is valid iff it was checked and has no crossing and no overlap.  Edges of different objects
are never compared.  Still the same one synchronisation; with `validity=False` the launches are the ones without it.

`predict(..., outlines=True, conflicts=True)` does compare them: it appends one `SceneConflicts` per stage the call has, after
the `SceneValidity` entries and last of all, in the same order (raw, simplified, regularised).  `c3d_rings_conflicts` bins the
edges of the whole table into a grid of cells on the device and counts, per object, the crossings, the collinear overlaps that
run the same way or the opposite way, and the touches of its edges with those of every other object; an object is in conflict
iff it was checked and has a crossing or a same-direction overlap.  Raw traced rings never conflict; the pieces of `split=R`
simplified ring by ring usually do.  Still the same one synchronisation; with `conflicts=False` the launches are the ones
without it.

`SceneInferencer(..., tta="hflip" | "flips" | "d4" | codes)` is test-time augmentation: every tile is predicted under a set of
the eight flips and rotations of the square, each view is undone on the output and the views are averaged before the
stitch.  A view code `v` in 0..7 transposes the tile if `v & 4`, then reverses its rows if `v & 2`, then its columns if
`v & 1`; a set is taken in ascending code order.  `c3d_scene_gather_views` cuts a tile under all views of the set at once
(one read of the scene), the model sees `batch // nv` tiles times `nv` views per forward, and `c3d_scene_fold_views` writes
the mean of the inverted views of every head straight into that head's ring slots -- it replaces the ring copy.  Averaged
are the maps the stitch blends: the BCD probability, the SCD logits and change probability, the BDA damage logits and
localisation probability; masks and argmax come after, from the stitch.  Still one upload and one synchronisation.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .data.transforms import BCDTransforms

AxisPlan = namedtuple("AxisPlan", "extent tile stride margin n k starts")
# labels i32 [Hs, Ws]; table i32 [max_objects, 8] = (area, x0, y0, x1, y1, cls, first, score_q); counts i32 [2] = (found, rows
# written); object_cls u8 [Hs, Ws]; hist i32 [max_objects, num_class] or None (BCD has no class map)
SceneObjects = namedtuple("SceneObjects", "labels table counts object_cls hist")


class SceneSplitObjects(SceneObjects):
    """The `SceneObjects` of `predict(objects=True, split=R)`: the same five fields, so everything that takes a `SceneObjects`
    takes it, plus `.info` i32 [4] = (status, seeds, growth rounds used, 0) of `c3d_scene_split`."""

    def __new__(cls, labels, table, counts, object_cls, hist, info):
        self = super().__new__(cls, labels, table, counts, object_cls, hist)
        self.info = info
        return self


REGION_MODES = ("pre", "post", "transition")


class SceneRegionObjects(SceneObjects):
    """The `SceneObjects` of `predict(objects=True, regions=mode)` (SCD): the regions of equal class of a class map instead of the
    components of the change mask, in the same five fields (`table[:, 5]` is the region's key, exact; `object_cls` is the key
    painted over the kept regions; `hist` is None), plus `.key_map` u8 [Hs, Ws], the map that was labelled -- the sieved one
    with `sieve=N` --, and `.info` i32 [8] of `c3d_regions_sieve` (zeros without `sieve`).  The key is the class of the chosen
    side, or `pre * num_class + post` for `"transition"` (`region_classes` decodes it)."""

    def __new__(cls, labels, table, counts, object_cls, hist, key_map, info):
        self = super().__new__(cls, labels, table, counts, object_cls, hist)
        self.key_map = key_map
        self.info = info
        return self


def region_classes(key, mode, num_class):
    """(from, to) of a region key (an int or an integer array): the class on its own side and 0 on the other for `"pre"` /
    `"post"`, `key // num_class` and `key % num_class` for `"transition"`."""
    if mode == "transition":
        return key // num_class, key % num_class
    return (key, key * 0) if mode == "pre" else (key * 0, key)
# rings i32 [max_rings, 8] = (id, start, n_vertices, area, perimeter, x, y, 0) in the order of their starting edge; vertices i32
# [max_vertices, 2] = (vx, vy) lattice points, ring after ring; counts i32 [5] = (rings found, rows written, vertices found,
# vertices written, status: _lib.OUTLINE_ST_*)
SceneOutlines = namedtuple("SceneOutlines", "rings vertices counts")
# `predict(..., simplify=tol, simplify_shared=True)`: rings, vertices and counts as the simplified SceneOutlines has them (vertices
# has twice the rows, (x, y) of a row is the ring's first vertex); left i32 [2 max_vertices] = the label left of the edge that
# leaves each vertex, the object being on the right; info i32 [8] = (nodes inserted, node vertices, arcs, closed arcs, arcs with a
# neighbour, collapsed rings, 0, 0)
SceneSharedOutlines = namedtuple("SceneSharedOutlines", "rings vertices counts left info")


class SceneSafeOutlines(SceneSharedOutlines):
    """The `SceneSharedOutlines` of `predict(..., simplify_shared=True, simplify_safe=True)`: the same five fields, so everything
    that takes a `SceneSharedOutlines` takes it, plus `.level` i32 [2 max_vertices] = the level of the arc of the edge leaving
    each vertex and `.safe` i64 [8] = (rounds run, rounds that raised, arcs with level > 0, arcs at the cap, defective pairs in
    round 0, in the last round, defective rings in round 0, status: `ops.outlines_simplify_safe`) of `c3d_outlines_simplify_safe`.  The two are attributes
    of the instance, as `SceneSplitObjects.info` is: `_replace`, `_make` and slices give a plain tuple of the five fields."""

    def __new__(cls, rings, vertices, counts, left, info, level, safe):
        self = super().__new__(cls, rings, vertices, counts, left, info)
        self.level, self.safe = level, safe
        return self


# the simplified rings filled back into pixels (`c3d_rings_fill`) and joined to the raw objects (`c3d_objects_match`, prediction =
# the raw objects): labels, table [max_objects, 8] and counts [2] as in SceneObjects; info i32 [4] = (status, ring rows used, K,
# 0); match = (match_raw i32 [max_objects, 4], match_filled i32 [max_objects, 4], conf, counts i64 [6], sum_iou f64 [1])
SceneFill = namedtuple("SceneFill", "labels table counts info match")
# `predict(..., shapes=True)`: the convex hull and the minimum-area rectangle of every object (`ops.rings_hull`): hulls i32
# [max_objects, 8], vertices i32 [., 2], rects i64 [max_objects, 8], counts i32 [5]
SceneShapes = namedtuple("SceneShapes", "hulls vertices rects counts")
# `predict(..., regularize=True)`: the simplified rings squared to the axes of their object's minimum-area rectangle
# (`ops.rings_regularize`): rings i32 [max_rings, 8] = (id, start, n, regularised?, perimeter, x, y, simplified n), vertices in
# units of 2^-REGULAR_FRAC_BITS pixel, counts i32 [5]
SceneRegular = namedtuple("SceneRegular", "rings vertices counts")
# `predict(..., validity=True)`: the crossings, overlaps and touches among the edges of every object of one ring table
# (`ops.rings_valid`): valid i64 [max_objects, 8] = (flag, rings, m, degenerate, cross, overlap, touch_vv, touch_ve), counts i64
# [8] = (checked, invalid, empty, incomplete, over work, sum cross, sum overlap, status).  An object is valid iff flag == 0 and
# cross == overlap == 0
SceneValidity = namedtuple("SceneValidity", "valid counts")
# `predict(..., conflicts=True)`: the crossings, overlaps and touches between the edges of different objects of one ring table
# (`ops.rings_conflicts`): conflict i64 [max_objects, 8] = (flag, partner, m, cross, same, opposite, touch_vv, touch_ve), counts
# i64 [8] = (checked, in conflict, empty, incomplete, over work, sum cross, sum same, status), info i64 [8] = (live edges, cell
# shift, cells_x, cells_y, entries, work, sum opposite, sum touches).  An object is in conflict iff flag == 0 and cross + same > 0
SceneConflicts = namedtuple("SceneConflicts", "conflict counts info")
REGULAR_FRAC_BITS = 4
TASKS = ("bcd", "scd", "bda")
WINDOWS = ("hann", "flat")
VIEW_SETS = {"none": (0,), "hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def view_codes(tta):
    """The ascending view codes of `tta`: one of the names of VIEW_SETS, or a sequence of codes in 0..7 (repeats count once)."""
    if isinstance(tta, str):
        if tta not in VIEW_SETS:
            raise ValueError(f"tta must be one of {tuple(VIEW_SETS)} or a sequence of view codes, got {tta!r}")
        return VIEW_SETS[tta]
    try:
        codes = [v for v in tta]
    except TypeError:
        raise ValueError(f"tta must be one of {tuple(VIEW_SETS)} or a sequence of view codes, got {tta!r}") from None
    if not codes or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 7 for v in codes):
        raise ValueError(f"view codes must be integers in 0..7 and at least one, got {tta!r}")
    return tuple(sorted({int(v) for v in codes}))


def view_mask(codes):
    """Bit mask of a set of view codes, as c3d_scene_gather_views and c3d_scene_fold_views take it."""
    mask = 0
    for v in codes:
        mask |= 1 << v
    return mask


def axis_plan(extent, tile, stride):
    """Tiling of one axis: margin, tile count, ring depth and the (possibly negative) start of every tile."""
    extent, tile, stride = int(extent), int(tile), int(stride)
    if extent < 1 or tile < 1:
        raise ValueError(f"extent and tile must be positive, got {extent} and {tile}")
    if stride < 1 or stride > tile:
        raise ValueError(f"stride must satisfy 1 <= stride <= tile = {tile}, got {stride}")
    if (tile - stride) % 2:
        raise ValueError(f"tile - stride must be even (the margin is (tile - stride) / 2), got {tile} - {stride}")
    margin, n = (tile - stride) // 2, -(-extent // stride)
    return AxisPlan(extent, tile, stride, margin, n, -(-tile // stride), np.arange(n, dtype=np.int64) * stride - margin)


def reflect_index(coord, extent):
    """numpy `reflect` for any overhang: period 2 * (extent - 1), the edge pixel is not repeated; extent 1 maps to 0."""
    c = np.asarray(coord, dtype=np.int64)
    if extent == 1:
        return np.zeros_like(c)
    period = 2 * (extent - 1)
    c = np.mod(c, period)
    return np.where(c >= extent, period - c, c)


def window_vector(name, tile):
    """One axis of the separable blending window, computed in float64 and rounded to f32 once: `flat` = ones, `hann` =
    sin^2(pi * (i + 0.5) / tile), which is strictly positive."""
    if name == "flat":
        return np.ones(tile, dtype=np.float32)
    if name == "hann":
        return (np.sin(np.pi * (np.arange(tile, dtype=np.float64) + 0.5) / tile) ** 2).astype(np.float32)
    raise ValueError(f"window must be one of {WINDOWS}, got {name!r}")


def strip_rows(plan, row):
    """Scene rows [y0, y1) that are final once tile row `row` exists: [row*s - m, (row+1)*s - m) clipped to the scene; the
    last tile row also closes the scene.  Empty (y1 <= y0) while the margin still reaches above the scene."""
    y0 = max(row * plan.stride - plan.margin, 0)
    y1 = plan.extent if row == plan.n - 1 else min((row + 1) * plan.stride - plan.margin, plan.extent)
    return y0, max(y1, y0)


def upload_windows(window, th, tw, device):
    return torch.from_numpy(window_vector(window, th)).to(device), torch.from_numpy(window_vector(window, tw)).to(device)


class SceneStitcher:
    """The ring of `k` tile rows of one output head and its strips: `put` copies predictions of consecutive tiles of one
    tile row into the ring, `stitch(row)` writes the rows that row completed."""

    def __init__(self, py, px, channels, window, device, blend=False, cls=True, windows=None):
        """`windows` = (wy, wx) device vectors that are already uploaded (SceneInferencer keeps one pair per device)."""
        self.py, self.px, self.C = py, px, int(channels)
        nbytes = py.k * px.n * self.C * py.tile * px.tile * 4
        if nbytes >= 2 ** 31:
            raise L.Change3DHipError(f"the stitch ring needs {nbytes} bytes ({py.k} tile rows x {px.n} tiles x {self.C} channels): "
                                     f"it must stay under 2 GiB; use a larger stride or split the scene into column bands")
        self.ring = torch.empty((py.k, px.n, self.C, py.tile, px.tile), dtype=torch.float32, device=device)
        self.wy, self.wx = windows if windows is not None else upload_windows(window, py.tile, px.tile, device)
        self.blend = torch.empty((self.C, py.extent, px.extent), dtype=torch.float32, device=device) if blend else None
        self.cls = torch.empty((py.extent, px.extent), dtype=torch.uint8, device=device) if cls else None

    def put(self, row, col, values):
        self.ring[row % self.py.k, col:col + values.shape[0]].copy_(values.reshape(values.shape[0], self.C, self.py.tile, self.px.tile))

    def fold(self, row, col, values, mask):
        """`put` for test-time augmentation: `values` holds every tile under the views of `mask`, tile-major; their mean with
        the views undone goes into the ring slots, no copy follows."""
        nv = ops.view_count(mask)
        ops.scene_fold_views(values.contiguous(), self.ring[row % self.py.k, col:col + values.shape[0] // nv], values.shape[0] // nv,
                             self.C, self.py.tile, self.px.tile, mask)

    def stitch(self, row, gate=None):
        ops.scene_stitch(self.ring, self.wy, self.wx, self.blend, self.cls, self.py.extent, self.px.extent, self.C, self.py.tile,
                         self.px.tile, self.py.stride, self.px.stride, row, gate=gate)


class SceneInferencer:
    """`SceneInferencer(model, task).predict(scene_u8)`: `task` is "bcd", "scd" or "bda", `stride` defaults to half the tile (an
    int, or a (y, x) pair), `window` is "hann" or "flat", `batch` tiles go through the model per forward.

    BCD returns `(prob f32 [Hs, Ws], mask u8 [Hs, Ws])` with mask = blended prob > 0.5.  SCD returns `(pre_cls, post_cls,
    change)` u8 maps: the class maps are the argmax of the blended logits multiplied by the change mask, the reference's
    validation post-processing (reference scripts/train_SCD.py:148-154).  BDA returns `(loc_prob f32 [Hs, Ws], loc_mask u8,
    damage_map u8, cls_logits f32 [num_class, Hs, Ws])` with damage_map = argmax of the blended logits times loc_mask.
    `objects=True` appends a `SceneObjects`: the objects of the mask (BCD, score = prob), of the change mask voted over
    `post_cls` (SCD), or the buildings of `loc_mask` voted over `damage_map` (BDA, score = loc_prob); classes from 1 vote.
    `outlines=True` (with `objects=True`) appends a `SceneOutlines` after it: the polygon rings of those objects.  `max_rings`
    and `max_vertices` default to `ops.scene_outlines_defaults`: 4 rings per row of the object table and 16 vertices per ring,
    cut to Hs * Ws and 4 * Hs * Ws.  The worst case, a 4-connected checkerboard, has Hs * Ws / 2 rings and 2 * Hs * Ws
    vertices; a scene past the limits sets `OUTLINE_ST_TRUNCATED` in `counts[4]` and keeps a prefix of its rings.
    `simplify=tol` (with `outlines=True`) appends one more `SceneOutlines`: the rings simplified with a tolerance of `tol`
    pixels in [0, 1024] (`ops.outlines_simplify`); column 3 of its rows is twice the signed area of the simplified ring and
    column 7 the ring's raw vertex count.  With `simplify=None` the result is the one without the argument.
    `simplify_shared=True` (with `simplify=tol`) puts a `SceneSharedOutlines` there instead (`ops.outlines_simplify_shared`): walls
    between objects are simplified once for both neighbours; `simplify_check`, `shapes`, `regularize`, `validity` and `conflicts`
    take it unchanged.  With `simplify_shared=False` the launches are the ones without the argument.
    `simplify_safe=True` (with `simplify_shared=True`) puts a `SceneSafeOutlines` there (`ops.outlines_simplify_safe`): the shared
    call in at most `safe_rounds` rounds (default 8, in [1, 64]) that give the arcs of every defect a smaller tolerance; its
    `.safe[7]` is 0 iff a round found nothing.  With `simplify_safe=False` the launches are the ones without the argument.
    `simplify_check=True` (with `simplify=tol`) appends a `SceneFill`: the simplified rings filled back into pixels
    (`ops.rings_fill`) and matched to the raw objects (`ops.objects_match`, raw objects first, threshold 0.5): row id-1 of
    `match[0]` is (partner id, intersection, union, covered) of raw object `id`.  With `simplify_check=False` the launches are
    the ones without the argument.
    `split=R` (with `objects=True`) splits touching objects (`ops.scene_split`): the mask is eroded by R pixels, in (0, 1024], and
    the components of what is left grow back inside the mask; the appended object is a `SceneSplitObjects`, a `SceneObjects`
    with `.info` = (status, seeds, rounds used, 0) that outlines, simplification, votes and `ObjectEvaluator` take unchanged.
    `split_rounds` (default 32) limits the growth rounds: `info[0] & SPLIT_ST_NOT_CONVERGED` says that it was too small.  With
    `split=None` the launches are the ones without the argument.
    `regions="pre" | "post" | "transition"` (SCD, with `objects=True`, not with `split`) labels the regions of equal class of a
    class map instead of the components of the change mask (`ops.scene_regions`): the key map is `pre_cls`, `post_cls` or
    `pre_cls * num_class + post_cls` (num_class <= 16), the appended object a `SceneRegionObjects`, a `SceneObjects` with
    `.key_map` and `.info` whose labels every later stage takes unchanged.  `min_area` still drops; `sieve=N` (in [1, 2^20])
    has the regions below N pixels absorbed by the neighbour with the longest border first (`ops.regions_sieve`), in at most
    `sieve_rounds` (default 8) rounds: `info[0] & SIEVE_ST_NOT_CONVERGED` says that it was too small.  With `regions=None` the
    launches are the ones without the argument.
    `shapes=True` (with `outlines=True`) appends a `SceneShapes` last: the convex hull and the minimum-area rectangle of every
    object (`ops.rings_hull`), taken from the raw rings -- also with `simplify=tol` -- and from the pieces with `split=R`.  Its
    `hulls` rows are a ring table that `ops.rings_fill` takes.  With `shapes=False` the launches are the ones without it.
    `regularize=True` (with `simplify=tol`) appends a `SceneRegular` after all of those: the simplified rings with every edge
    parallel or perpendicular to the chosen rectangle edge of their object (`ops.rings_regularize` on the hulls of the raw
    rings, the one `ops.rings_hull` call that `shapes=True` makes, shared when both are asked for), coordinates in sixteenths of
    a pixel.  `regularize_check=True` appends a `SceneFill` after it: those rings filled at 1/16 px and matched to the raw
    objects, as `simplify_check` does for the simplified ones.  With `regularize=False` the launches are the ones without it.
    `validity=True` (with `outlines=True`) appends, last of all, a `SceneValidity` of the raw rings, one of the simplified rings
    with `simplify=tol` and one of the regularised rings with `regularize=True` (`ops.rings_valid`): per object its crossings,
    overlaps and touches.  With `validity=False` the launches are the ones without it.
    `conflicts=True` (with `outlines=True`) appends, after those and last of all, a `SceneConflicts` per stage in the same order
    (`ops.rings_conflicts`): per object its crossings, overlaps and touches with every other object.  With `conflicts=False` the
    launches are the ones without it.
    `tta` is None, a name of `VIEW_SETS` ("none", "hflip", "flips", "d4") or a sequence of view codes: the tiles are predicted
    under those `nv` views and averaged with the views undone (module docstring).  `batch` stays the number of model inputs
    per forward, so a forward takes `batch // nv` tiles; a transposing view (codes 4..7) needs a square model input.  With
    `tta=None` nothing changes.
    All results stay on the device."""

    def __init__(self, model, task, stride=None, window="hann", batch=32, mean=BCDTransforms.DEFAULT_MEAN,
                 std=BCDTransforms.DEFAULT_STD, tta=None):
        if task not in TASKS:
            raise ValueError(f"task must be one of {TASKS}, got {task!r}")
        if task == "bda" and not (hasattr(model, "decoder_loc") and hasattr(model, "decoder_cls")):
            raise ValueError("task 'bda' needs a model with the localisation and damage heads (num_perception_frame = 2)")
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        self.model, self.task, self.window, self.batch = model.eval(), task, window, int(batch)
        self.th, self.tw = int(model.args.in_height), int(model.args.in_width)
        sy, sx = (stride, stride) if not isinstance(stride, (tuple, list)) else stride
        self.sy, self.sx = int(self.th // 2 if sy is None else sy), int(self.tw // 2 if sx is None else sx)
        axis_plan(self.th, self.th, self.sy), axis_plan(self.tw, self.tw, self.sx)      # refuse a bad stride here
        self.views = None if tta is None else view_codes(tta)
        if self.views is not None:
            if self.views[-1] >= 4 and self.th != self.tw:
                raise ValueError(f"tta views {self.views} transpose the tile: the model input must be square, got {self.th} x {self.tw}")
            if self.batch < len(self.views):
                raise ValueError(f"batch = {self.batch} model inputs per forward cannot hold one tile under {len(self.views)} views")
        self.num_class = int(model.args.num_class)
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self._consts, self._origins = {}, {}             # device tables: uploaded once, not per scene

    def _constants(self, dev):
        """(mean, std, wy, wx) on `dev`: uploads from pageable memory block the host, so they happen once per device."""
        if dev not in self._consts:
            self._consts[dev] = (torch.tensor(self.mean, device=dev), torch.tensor(self.std, device=dev),
                                 *upload_windows(self.window, self.th, self.tw, dev))
        return self._consts[dev]

    def _origin_table(self, py, px, dev):
        """i32 [n, 2] of (y, x) tile starts in row-major tile order; one upload per scene size and device."""
        key = (py.extent, px.extent, dev)
        if key not in self._origins:
            origins = np.stack([np.repeat(py.starts, px.n), np.tile(px.starts, py.n)], axis=1).astype(np.int32)
            self._origins[key] = torch.from_numpy(origins).to(dev)
        return self._origins[key]

    def _device(self):
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise L.Change3DHipError(f"the model is on {dev}: whole-scene inference runs only as HIP kernels on an MI355X "
                                     f"(no CPU fallback)")
        return dev

    @torch.no_grad()
    def predict(self, scene_u8, objects=False, min_area=1, connectivity=8, max_objects=65536, outlines=False, max_rings=None,
                max_vertices=None, simplify=None, split=None, split_rounds=None, simplify_check=False, shapes=False,
                regularize=False, regularize_check=False, validity=False, conflicts=False, simplify_shared=False, simplify_safe=False,
                safe_rounds=None, regions=None, sieve=None, sieve_rounds=None):
        if regions is not None:
            if regions not in REGION_MODES:
                raise ValueError(f"regions must be one of {REGION_MODES}, got {regions!r}")
            if self.task != "scd":
                raise ValueError(f"regions={regions!r} labels the class maps of SCD: the task is {self.task}")
            if not objects:
                raise ValueError("regions=mode chooses what objects=True labels: it needs objects=True")
            if split is not None:
                raise ValueError("regions=mode and split=R both replace the labelling: give one of them")
            if regions == "transition" and self.num_class > 16:
                raise ValueError(f"regions='transition' keys a region by pre * num_class + post in a byte: num_class = "
                                 f"{self.num_class} is above 16")
        if sieve is None and sieve_rounds is not None:
            raise ValueError("sieve_rounds limits the rounds of sieve=N: it needs sieve")
        if sieve is not None:
            if regions is None:
                raise ValueError("sieve=N absorbs the small regions of regions=mode: it needs regions")
            sieve_rounds = 8 if sieve_rounds is None else int(sieve_rounds)
            if not 1 <= int(sieve) <= 2 ** 20 or not 1 <= sieve_rounds <= 65536:
                raise ValueError(f"sieve must lie in [1, 2^20] and sieve_rounds in [1, 65536], got {sieve} and {sieve_rounds}")
        if outlines and not objects:
            raise ValueError("outlines=True traces the objects of the map: it needs objects=True")
        if validity and not outlines:
            raise ValueError("validity=True tests the traced rings of the objects: it needs outlines=True")
        if conflicts and not outlines:
            raise ValueError("conflicts=True compares the traced rings of different objects: it needs outlines=True")
        if shapes and not outlines:
            raise ValueError("shapes=True takes the hulls and rectangles of the traced rings: it needs outlines=True")
        if split is None and split_rounds is not None:
            raise ValueError("split_rounds limits the growth rounds of split=R: it needs split")
        if split is not None:
            if not objects:
                raise ValueError("split=R splits the objects of the map: it needs objects=True")
            ops.boundary_radius2(split)                 # raises outside (0, 1024] before anything is enqueued
            split_rounds = 32 if split_rounds is None else int(split_rounds)
            if not 1 <= split_rounds <= 65536:
                raise ValueError(f"split_rounds must lie in [1, 65536], got {split_rounds}")
        if simplify is not None:
            if not outlines:
                raise ValueError("simplify=tol simplifies the outlines of the objects: it needs outlines=True")
            ops.simplify_tol2_q(simplify)               # raises outside [0, 1024] before anything is enqueued
        if simplify_shared and simplify is None:
            raise ValueError("simplify_shared=True chooses how simplify=tol simplifies: it needs simplify")
        if simplify_safe and not simplify_shared:
            raise ValueError("simplify_safe=True refines the arcs of simplify_shared=True: it needs simplify_shared")
        if safe_rounds is not None and not simplify_safe:
            raise ValueError("safe_rounds limits the rounds of simplify_safe=True: it needs simplify_safe")
        if simplify_safe:
            safe_rounds = 8 if safe_rounds is None else int(safe_rounds)
            if not 1 <= safe_rounds <= 64:
                raise ValueError(f"safe_rounds must lie in [1, 64], got {safe_rounds}")
        if simplify_check and simplify is None:
            raise ValueError("simplify_check=True measures what simplify=tol cost: it needs simplify")
        if regularize and simplify is None:
            raise ValueError("regularize=True squares the simplified rings: it needs simplify")
        if regularize_check and not regularize:
            raise ValueError("regularize_check=True measures what regularize=True cost: it needs regularize")
        if any(v is not None and int(v) < 1 for v in (max_rings, max_vertices)):
            raise ValueError(f"max_rings and max_vertices must be positive, got {max_rings} and {max_vertices}")
        dev = self._device()
        if connectivity not in (4, 8) or int(max_objects) < 1:
            raise ValueError(f"connectivity must be 4 or 8 and max_objects positive, got {connectivity} and {max_objects}")
        scene = torch.as_tensor(scene_u8)
        if scene.dtype != torch.uint8 or scene.dim() != 3 or scene.shape[-1] != 6:
            raise ValueError("scene must be uint8 [Hs, Ws, 6] (pre RGB | post RGB)")
        L.lib()
        scene = scene.to(dev).contiguous()                                            # the one upload
        Hs, Ws = int(scene.shape[0]), int(scene.shape[1])
        py, px = axis_plan(Hs, self.th, self.sy), axis_plan(Ws, self.tw, self.sx)
        n = py.n * px.n
        origins = self._origin_table(py, px, dev)
        mean, std, wy, wx = self._constants(dev)
        if self.task == "bcd":
            heads = [SceneStitcher(py, px, 1, self.window, dev, blend=True, windows=(wy, wx))]
        elif self.task == "bda":                        # update_bda's order: damage logits, localisation probability
            heads = [SceneStitcher(py, px, C, self.window, dev, blend=True, windows=(wy, wx)) for C in (self.num_class, 1)]
        else:
            heads = [SceneStitcher(py, px, C, self.window, dev, windows=(wy, wx)) for C in (self.num_class, self.num_class, 1)]
        mask, nv = (0, 1) if self.views is None else (view_mask(self.views), len(self.views))
        nb = min(self.batch // nv, n)                   # tiles per forward; each under nv views
        pre = torch.empty((nb * nv, 3, self.th, self.tw), dtype=torch.float32, device=dev)
        post = torch.empty_like(pre)
        for j0 in range(0, n, nb):
            b = min(nb, n - j0)
            if mask:
                ops.scene_gather_views(scene, origins[j0:j0 + b], mean, std, pre, post, Hs, Ws, b, self.th, self.tw, mask)
            else:
                ops.scene_gather(scene, origins[j0:j0 + b], mean, std, pre, post, Hs, Ws, b, self.th, self.tw)
            out = getattr(self.model, "update_" + self.task)(pre[:b * nv], post[:b * nv])
            outs = [out] if self.task == "bcd" else list(out)
            j = j0
            while j < j0 + b:                           # the batch, one tile row at a time: a strip goes out once its row is whole
                row, col = divmod(j, px.n)
                cnt = min(px.n - col, j0 + b - j)
                for head, o in zip(heads, outs):
                    if mask:
                        head.fold(row, col, o[(j - j0) * nv:(j - j0 + cnt) * nv].float(), mask)
                    else:
                        head.put(row, col, o[j - j0:j - j0 + cnt].float())
                if col + cnt == px.n:
                    if self.task == "bcd":
                        heads[0].stitch(row)
                    elif self.task == "bda":
                        heads[1].stitch(row)
                        heads[0].stitch(row, gate=heads[1].cls)
                    else:
                        heads[2].stitch(row)
                        heads[0].stitch(row, gate=heads[2].cls)
                        heads[1].stitch(row, gate=heads[2].cls)
                j += cnt
        if self.task == "bcd":
            result = (heads[0].blend[0], heads[0].cls)
            found = dict(mask=heads[0].cls, score=heads[0].blend[0])
        elif self.task == "bda":
            result = (heads[1].blend[0], heads[1].cls, heads[0].cls, heads[0].blend)
            found = dict(mask=heads[1].cls, cls_map=heads[0].cls, score=heads[1].blend[0], n_cls=self.num_class)
        else:
            result = (heads[0].cls, heads[1].cls, heads[2].cls)
            found = dict(mask=heads[2].cls, cls_map=heads[1].cls, n_cls=self.num_class)
        if objects:
            if regions is not None:
                if regions == "transition":             # < 256 with num_class <= 16
                    key_map = (heads[0].cls.to(torch.int16) * self.num_class + heads[1].cls).to(torch.uint8)
                else:
                    key_map = heads[0].cls if regions == "pre" else heads[1].cls
                info = torch.zeros(8, dtype=torch.int32, device=dev)
                if sieve is not None:
                    labels, table, _, key_map, counts, info = ops.regions_sieve(key_map, int(sieve), connectivity=connectivity,
                                                                                max_rounds=sieve_rounds, max_objects=max_objects)
                    object_key = key_map                # every nonzero pixel lies in a region with a label
                if sieve is None or int(min_area) > 1:  # min_area drops, as everywhere
                    labels, table, _, object_key, counts = ops.scene_regions(key_map, connectivity=connectivity, min_area=min_area,
                                                                             max_objects=max_objects)
                result += (SceneRegionObjects(labels, table, counts, object_key, None, key_map, info),)
            elif split is not None:
                labels, table, hist, object_cls, counts, info = ops.scene_split(
                    found.pop("mask"), split, first_class=1, connectivity=connectivity, min_area=min_area, max_objects=max_objects,
                    max_rounds=split_rounds, **found)
                result += (SceneSplitObjects(labels, table, counts, object_cls, hist, info),)
            else:
                labels, table, hist, object_cls, counts = ops.scene_objects(first_class=1, connectivity=connectivity,
                                                                            min_area=min_area, max_objects=max_objects, **found)
                result += (SceneObjects(labels, table, counts, object_cls, hist),)
            if outlines:
                result += (SceneOutlines(*ops.scene_outlines(labels, counts, connectivity=connectivity, max_objects=max_objects,
                                                             max_rings=max_rings, max_vertices=max_vertices)),)
                raw = result[-1]
                if simplify is not None:
                    if simplify_safe:
                        result += (SceneSafeOutlines(*ops.outlines_simplify_safe(labels, counts, *raw, simplify, max_rounds=safe_rounds,
                                                                                 max_objects=max_objects)),)
                    elif simplify_shared:
                        result += (SceneSharedOutlines(*ops.outlines_simplify_shared(labels, counts, *raw, simplify,
                                                                                     max_objects=max_objects)),)
                    else:
                        result += (SceneOutlines(*ops.outlines_simplify(*raw, simplify)),)
                    simple = result[-1][:3]             # what every later stage takes
                    if simplify_check:
                        f_labels, f_table, f_counts, _, _, f_info = ops.rings_fill(*simple, Hs, Ws, max_objects=max_objects)
                        match = ops.objects_match(labels, table, counts, f_labels, f_table, f_counts, n_cls=1, iou_thr=0.5)
                        result += (SceneFill(f_labels, f_table, f_counts, f_info, match),)
                hull = ops.rings_hull(*raw, max_objects=max_objects) if shapes or regularize else None   # one call for both
                if shapes:                              # of the raw rings, whatever else was asked for
                    result += (SceneShapes(*hull),)
                if regularize:                          # the simplified rings along the rectangle edge of the raw object
                    result += (SceneRegular(*ops.rings_regularize(*simple, *hull, frac_bits=REGULAR_FRAC_BITS)),)
                    if regularize_check:
                        f_labels, f_table, f_counts, _, _, f_info = ops.rings_fill(*result[-1], Hs, Ws, frac_bits=REGULAR_FRAC_BITS,
                                                                                   max_objects=max_objects)
                        match = ops.objects_match(labels, table, counts, f_labels, f_table, f_counts, n_cls=1, iou_thr=0.5)
                        result += (SceneFill(f_labels, f_table, f_counts, f_info, match),)
                    regular = result[-2] if regularize_check else result[-1]
                if validity:                            # last, so that no position above moves: raw, simplified, regularised
                    result += (SceneValidity(*ops.rings_valid(*raw, max_objects=max_objects)),)
                    if simplify is not None:
                        result += (SceneValidity(*ops.rings_valid(*simple, max_objects=max_objects)),)
                    if regularize:
                        result += (SceneValidity(*ops.rings_valid(*regular, frac_bits=REGULAR_FRAC_BITS, max_objects=max_objects)),)
                if conflicts:                           # after the validity entries, in the same order
                    result += (SceneConflicts(*ops.rings_conflicts(*raw, max_objects=max_objects)),)
                    if simplify is not None:
                        result += (SceneConflicts(*ops.rings_conflicts(*simple, max_objects=max_objects)),)
                    if regularize:
                        result += (SceneConflicts(*ops.rings_conflicts(*regular, frac_bits=REGULAR_FRAC_BITS, max_objects=max_objects)),)
        torch.cuda.current_stream().synchronize()       # the one host synchronisation after the scene's upload
        return result
