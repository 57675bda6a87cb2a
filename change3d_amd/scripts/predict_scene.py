"""Change maps of whole scenes: `python -m change3d_amd.scripts.predict_scene --task BCD --weights best_model.pth
--pre A.png --post B.png`, or `--file_root DIR --split test` for the reference's directory layout
(`<root>/<split>/{t1,t2,label}` for BCD, `{t1,t2,label1,label2,change}` for SCD, xBD's `{t1,t2,label1,label2}` for
`--task BDA`; change3d_amd/data/dataset.py).

The reference has no such step: its scripts stop at `val()` over pre-cut crops of the training size (reference
scripts/train_BCD.py:92-154, scripts/train_SCD.py:104-178).  A pair of any size is decoded with PIL, uploaded once as
uint8 and tiled, predicted and stitched on the GPU (change3d_amd/infer.py).  The mask (0 / 255) or the two class maps and
the change mask are written as PNG; where labels exist the scene's predictions go to the on-device confusion matrix (BCD)
or joint histogram (SCD) of the training mirrors and the reference's score line is printed
(scripts/train_BCD.py:364-370, scripts/train_SCD.py:172-176).  BDA writes `loc/<name>.png` (0 / 255) and
`damage/<name>.png`, and with labels prints the columns of `train_BDA.py`'s `val` from the device counts of
`c3d_bda_confusion`.

`--objects` adds `objects/<name>.csv`, one line per connected object of the mask (SCD: of the change mask, `cls` voted over
the post class map, no score) with at least `--min_area` pixels (`id,area,x0,y0,x1,y1,cls,score`), found on the device by
`c3d_scene_objects`; BDA also writes
`damage_objects/<name>.png`, the majority damage class of every building painted over its footprint, and scores it.

`--objects --polygons` adds `objects/<name>.geojson`: a `FeatureCollection` in pixel coordinates with one `Polygon` per object,
traced on the device by `c3d_scene_outlines` -- `[outline, hole, ...]`, every ring closed by repeating its first vertex, holes
in ring order -- with the CSV's `id, area, cls, score` and the outline's `perimeter` as properties.  An object whose rings did
not fit `--max_rings` / `--max_vertices` is left out and the run ends with an error that says so.
`--simplify TOL` (with `--polygons`) simplifies every ring on the device first (`c3d_outlines_simplify`, Douglas-Peucker with a
tolerance of TOL pixels): the coordinates then come from the simplified rings and each feature also gets `vertices_raw` and
`vertices`, its vertex counts before and after.  A ring whose simplified area is zero or has changed sign keeps its raw vertices.

`--simplify_check` (with `--simplify`) measures what the simplification cost, on the device: the simplified rings are filled back
into pixels (`c3d_rings_fill`: a pixel belongs to a polygon iff its centre lies inside, even-odd over the rings of an object) and
joined to the raw objects (`c3d_objects_match`, whose partners are unique because a pair needs an IoU above 0.5: an object that
drifted further has no partner and the IoU 0).  Every feature gets an `iou` property and the run ends with a line `simplify: tol
objects kept vanished iou_mean iou_min`: `kept` counts the objects whose partner is their own id, `vanished` those without a
pixel after the fill.  `--simplify_shared` (with `--simplify`) simplifies every wall between two objects once for both
(`c3d_outlines_simplify_shared`): the rings are cut at the points where three or more regions of the label map meet, each arc
between two such nodes is simplified on its own, and both neighbours get the same vertices.  Every feature gets `neighbours`, the
sorted ids on the other side of its walls, and `collapsed`; an object whose outline collapsed or changed the sign of its area is
written with `"geometry": null`, a hole that did is left out, and nothing ever falls back to raw vertices -- which is why the flag
is refused together with `--simplify_min_iou`, `--simplify_valid` and `--simplify_clean`.  The run ends with a line `shared: tol
= .. objects = .. nodes = .. arcs = .. shared_arcs = .. collapsed = ..`.  With `--regularize` the squared rings no longer share
their walls.  `--simplify_safe` (implies `--simplify_shared`, and is refused where that flag is) repairs what the shared rule
leaves: `c3d_outlines_simplify_safe` runs it in at most `--safe_rounds N` rounds (default 8) and gives every arc that takes part
in a defect -- edges that cross or overlap, a vertex inside another edge, a ring that collapsed or flipped -- a smaller tolerance
of its own, the same for both neighbours.  Every feature gets `refined`, the number of its arcs with a level above 0, and the run
ends with a line `safe: tol = .. rounds = .. raised = .. arcs_refined = .. arcs_raw = .. defects = <pairs in round 0> -> <in the
last round>` (rounds and raised: the most of any scene).  A scene that did not converge ends the run with an error that names
`--safe_rounds`, or the work cap.  `--simplify_min_iou F` implies the check and leaves every object whose IoU is not above F on its raw
vertices, in every ring.

`--shapes` (with `--polygons`) describes every object's shape, on the device (`c3d_rings_hull` on the raw rings): each feature
gains `hull_area`, `hull_vertices`, `solidity` = area / hull area, `rect_area`, `rect_long`, `rect_short`, `rect_angle` (the long
side's direction, degrees in [0, 180), y down) and `rectangularity` = area / area of the minimum-area rectangle; the hulls and
the rectangles go to `objects/<name>.hulls.geojson` and `objects/<name>.rects.geojson`, and the run ends with a line `shapes:
objects = .. solidity_mean = .. rectangularity_mean = ..`.

`--regularize` (with `--polygons --simplify TOL`) squares every simplified ring to the axes of its object's minimum-area rectangle,
on the device (`c3d_rings_regularize`), and writes `objects/<name>.regular.geojson`: the features and properties of
`objects/<name>.geojson` with coordinates at 1/16 px as floats and `regular` (true or false) per feature.  An object with a ring
that was copied, or whose regularised area is zero or has changed sign, keeps its simplified rings there (`regular: false`).
`--regularize_min_iou F` also fills the regularised polygons back into pixels and joins them to the raw objects: every feature of
that file gets `iou`, and an object whose IoU is not above F keeps its simplified rings.  Nothing else that the run writes or
prints changes; it ends with a line `regularize: objects = .. regular = .. fallback = .. iou_mean = .. iou_min = ..`.

`--label_polygons FILE` (BCD, BDA) takes the ground truth as polygons instead of a label raster: a GeoJSON `FeatureCollection`
in pixel coordinates, such as `--polygons` writes, or an xBD label JSON (change3d_amd/vector_labels.py); with `--file_root` it
names a directory holding `<name>.json` or `<name>.geojson`.  The polygons are filled on the device (`c3d_rings_fill`) and
everything that scores reads the result: the pixel scores its mask (BDA: and its class map), `--objects` its labels -- one
ground-truth object per feature, so two labelled buildings that touch stay two, where a raster would join them --, `--boundary`
its mask.

`--polygon_scores` (with `--label_polygons` and `--objects --polygons`) scores the predicted polygons against the labelled ones,
on the device (change3d_amd/polygon_metrics.py, `c3d_rings_polis`): for every predicted object that `--objects` matched to a
labelled one, PoLiS -- the mean distance of the vertices of either polygon to the boundary of the other, averaged over the two
directions -- and the largest of those vertex distances, in pixels, against the label's rings at 1/16 px.  That maximum is the
vertex-to-boundary Hausdorff distance, not the Hausdorff distance of the two boundaries, whose maximum may fall inside an edge.
Every stage the run has is scored: the raw rings, the simplified rings with `--simplify`, and the regularised rings as
`c3d_rings_regularize` left them with `--regularize`; the host-side fallbacks of `--simplify_min_iou` and `--regularize_min_iou`,
which only change the written files, are not reflected.  `objects/<name>.polis.csv` lists `stage,id,gt_id,n,n_gt,polis,hausdorff,
flag` per predicted object (flag 0 scored, 1 no partner, 2 an incomplete or empty polygon, 3 too large a pair), and the run ends
with one line per stage, `polygons[raw]: pairs polis hausdorff_mean hausdorff_max n_ratio skipped`: the means over the scored
pairs, `n_ratio` the mean of predicted over labelled vertices, `skipped` the matched pairs that were not scored.

`--validity` (with `--polygons`) tests every polygon against itself, on the device (`c3d_rings_valid`): proper crossings and
collinear overlaps among the edges of an object, holes included, make it invalid; touches are counted and never disqualify.
Every feature of `objects/<name>.geojson` gains `valid`, `crossings`, `overlaps` and `touches` of the simplified stage with
`--simplify`, else of the raw rings; every feature of `objects/<name>.regular.geojson` the same of the regularised stage.  The
run ends with one line per stage, `validity[raw|simplified|regular]: objects valid invalid unchecked crossings overlaps`; an
object that could not be checked (rings cut off, or more edge pairs than the call's work cap) is named there as
`<scene>:<id>` and counts as not valid.  `--simplify_valid` implies `--validity` and leaves every object that is not valid on
its raw vertices in every ring, as `--simplify_min_iou` does (with both, either one suffices); `--regularize_valid` leaves such
an object on its simplified rings with `regular: false`, beside `--regularize_min_iou`.  Edges of different objects are never
compared, and whether a hole lies inside its outline is not examined.

`--conflicts` (with `--polygons`) compares the polygons of different objects, on the device (`c3d_rings_conflicts`, a grid of edge
cells): an object is in conflict iff one of its edges properly crosses an edge of another object or overlaps one collinearly in
the same direction; overlaps in opposite directions are the shared walls of pieces that meet, and touches never count.  Every
feature of `objects/<name>.geojson` gains `conflicts` (crossings plus same-direction overlaps), `conflict_with` (the smallest id
it conflicts with, 0 if none) and `shared_walls` of the coordinates that are written; every feature of
`objects/<name>.regular.geojson` the same of the regularised stage.  The run ends with one line per stage,
`conflicts[raw|simplified|regular]: objects clean in_conflict unchecked crossings overlaps shared_walls`.  Raw traced rings never
conflict; the pieces of `--split_objects` simplified ring by ring usually do.  `--simplify_clean` implies `--conflicts` and puts
every object in conflict back on its raw vertices in every ring, beside `--simplify_min_iou` and `--simplify_valid` (any one
suffices).  A raw staircase can cross a neighbour's chord that the simplified ring did not, so the table that is about to be
written is assembled on the host, uploaded and checked again, and its objects in conflict fall back too, for at most
`--clean_rounds N` rounds (default 8; each is one more synchronisation, under this flag only).  The properties and the closing
line then describe what is written, and the line adds `rounds` (the most any scene took) and `remaining`; objects still in
conflict after N rounds are named `<scene>:<id>` and the run ends with an error.  `--regularize_clean` does the same for
`objects/<name>.regular.geojson`, falling back to what the main file writes for that object, with `regular: false`.  An object
that lies wholly inside another, and a boundary that passes through another exactly at a vertex, are not seen.

`--tta hflip|flips|d4` is test-time augmentation: every tile is predicted under the two mirror views, the four flips or all
eight flips and rotations of the square, each view is undone on the device and the views are averaged before the stitch
(`c3d_scene_gather_views`, `c3d_scene_fold_views`; change3d_amd/infer.py).  `--batch_size` stays the number of model inputs
per forward, so it must be at least the number of views; `d4` needs `--in_height` = `--in_width`.  The default `none` is the
plain path.  Everything downstream -- masks, objects, polygons, score lines -- takes the averaged map unchanged.

`--objects` with labels also scores the objects themselves (change3d_amd/object_metrics.py, `c3d_objects_match`): the
predicted objects against the objects of the label mask (BCD), of the change label voted over label2 (SCD) or the buildings
of `label_loc > 0` voted over `label_loc * label_cls` (BDA).  A pair matches iff its IoU is strictly above `--iou_thr`.  One
more line follows the score line, `objects: tp fp fn precision recall f1 sq rq pq` (BDA: and the object F1 per damage
class), and `objects/<name>.match.csv` lists `id,gt_id,inter,union,covered` per predicted object and, under a `# gt` line,
`id,pred_id,inter,union,covered` per ground-truth object.

`--boundary D` with labels scores how well the outlines fit (change3d_amd/boundary_metrics.py, `c3d_boundary_counts` on the exact
distance transform `c3d_scene_edt`): Boundary IoU over the bands of width D pixels, and the precision, recall and F1 of the
contour pixels with a tolerance of `--boundary_tol` pixels (default D), on the masks that `--objects` scores: the mask against
`label > 0` (BCD), the change mask against the change label (SCD), `loc_mask` against `label_loc > 0` (BDA).  One more line
follows the score lines, `boundary: d tol biou precision recall f1`.  Without labels the option does nothing.

`--objects --split_objects R` splits touching objects before anything else sees them (`c3d_scene_split`): the mask is eroded
by R pixels, the components of what is left are seeds, and every seed grows back inside the mask, so two footprints joined by
a neck narrower than about 2 R become two rows, two polygons and two votes.  (`--split` alone is the data set split of
`--file_root`.)  The growth runs at most `--split_rounds` rounds (default 32); a scene that needs more ends the run with an
error that says so.  The labels that `--objects` scores against are NOT split.
"""
import json
import os
import sys
from argparse import ArgumentParser, ArgumentTypeError
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from change3d_amd.data.dataset import BCDDataset, BDADataset, SCDDataset, read_label, read_rgb  # noqa: E402
from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops, vector_labels  # noqa: E402
from change3d_amd.infer import REGULAR_FRAC_BITS, SceneInferencer, region_classes  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from change3d_amd.boundary_metrics import BoundaryEvaluator  # noqa: E402
from change3d_amd.object_metrics import ObjectEvaluator  # noqa: E402
from change3d_amd.polygon_metrics import PolygonEvaluator  # noqa: E402
from change3d_amd.model.utils import BDAEvaluator, Evaluator, SCDHistogram, bda_scores  # noqa: E402
from change3d_amd.utils.metric_tool import ConfuseMatrixMeter  # noqa: E402


def num_classes(args):
    """--num_class, or the task's default: 7 SCD classes (SECOND), 5 BDA damage classes (xBD); BCD has one output."""
    if args.task == "BCD":
        return 1
    return args.num_class if args.num_class is not None else {"SCD": 7, "BDA": 5}[args.task]


def build_model(args, device):
    frames, dataset = {"BCD": (1, "LEVIR-CD"), "SCD": (3, "SECOND"), "BDA": (2, "xBD")}[args.task]
    margs = SimpleNamespace(pretrained=args.pretrained, num_perception_frame=frames, in_height=args.in_height,
                            in_width=args.in_width, dataset=dataset,
                            num_class=num_classes(args),
                            act_dtype=torch.bfloat16 if args.act_dtype == "bf16" else torch.float32)
    model = Trainer(margs)
    state = torch.load(args.weights, map_location="cpu")
    model.load_state_dict(state["state_dict"] if "state_dict" in state else state)
    return model.to(device)


def scenes(args):
    """(name, image uint8 [H, W, 6], label uint8 or None) per scene."""
    if args.file_root:
        ds = {"BCD": BCDDataset, "SCD": SCDDataset, "BDA": BDADataset}[args.task](args.file_root, args.split)
        for i, name in enumerate(ds.file_list):
            img, label = ds.raw(i)
            yield os.path.splitext(name)[0], img, label
        return
    pre, post = read_rgb(args.pre), read_rgb(args.post)
    if pre.shape != post.shape:
        raise ValueError(f"{args.pre} is {pre.shape[:2]} but {args.post} is {post.shape[:2]}")
    if args.task == "BDA":                                # cv2's channel order, as BDADataset reads the training pairs
        pre, post = pre[:, :, ::-1], post[:, :, ::-1]
    files = {"BCD": [args.label], "SCD": [args.label1, args.label2, args.change], "BDA": [args.label1, args.label2]}[args.task]
    label = None
    if all(files):
        labels = [read_label(f) for f in files]
        label = labels[0] if len(labels) == 1 else np.stack(labels, axis=2)
    yield "scene", np.concatenate((pre, post), axis=2), label


def save_png(path, array):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(array).save(path)


def save_objects(path, objects, regions=None, num_class=0):
    """One CSV line per table row; the one read-back of the table.  Returns (found, written).  `regions` (the mode of
    `--regions`): `cls` is the region's key, and every line ends with the `from` and `to` classes it stands for."""
    found, rows = (int(v) for v in objects.counts.cpu())
    table = objects.table[:rows].cpu().numpy()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("id,area,x0,y0,x1,y1,cls,score" + (",from,to" if regions else "") + "\n")
        for k, (area, x0, y0, x1, y1, cls, _, score_q) in enumerate(table.tolist()):
            ends = ",{},{}".format(*region_classes(cls, regions, num_class)) if regions else ""
            f.write(f"{k + 1},{area},{x0},{y0},{x1},{y1},{cls},{score_q / 65535:.4f}{ends}\n")
    if found > rows:
        print(f"{path}: {found} objects found, the table holds the first {rows} (max_objects)")
    return found, rows


EMPTY_ROW = (1, 0, 0, 0, 0, 0, 0, 0)                      # an id past the last one of the ring table: flag 1, nothing to check


def validity_properties(row):
    """The feature properties of one row of a `SceneValidity`: valid iff the object was checked and neither crosses nor overlaps
    itself; touches (vertex on vertex, vertex inside an edge) are reported and never disqualify."""
    flag, _, _, _, cross, overlap, touch_vv, touch_ve = (int(v) for v in row)
    return dict(valid=flag == 0 and cross == 0 and overlap == 0, crossings=cross, overlaps=overlap, touches=touch_vv + touch_ve)


def not_valid_ids(rows):
    """The ids of the rows of a `SceneValidity` (host array [rows, 8]) that are not valid; an unchecked object is one of them."""
    return {k + 1 for k, row in enumerate(np.asarray(rows).tolist()) if not validity_properties(row)["valid"]}


def polygons_geojson(table, rings, vertices, simplified=None, iou=None, min_iou=None, extra=None, validity=None, not_valid=None,
                     shared=None, refined=None):
    """(FeatureCollection dict, ids left out) from host arrays: `table` [rows, 8] of the objects, `rings` [ring rows, 8] and
    `vertices` [vertices written, 2] of their outlines.  An object is complete iff it has one ring of positive area, every
    ring of it has its vertices (start >= 0) and the signed areas add up to the table's area -- a hole ring cut off by
    max_rings leaves the sum too large.  Incomplete objects are left out.
    `simplified` = (rings, vertices) of `c3d_outlines_simplify` on the same table, row for row: the coordinates of a ring then
    come from the simplified list -- unless its doubled area there is zero or has the other sign than the raw area, or its row
    has no vertices, in which case the ring keeps its raw vertices -- and every feature gets the counts `vertices_raw` and
    `vertices`.  Completeness is judged on the raw rings either way.
    `iou` [rows] (with `simplified`): the IoU of every object with its simplified polygon filled back into pixels; each feature
    gets it as a property, and with `min_iou` an object whose IoU is not above it keeps its raw vertices in every ring.
    `extra`: id -> further properties of that object's feature (`--shapes`).
    `validity` [rows, 8]: the rows of `c3d_rings_valid` on the stage that is written (the simplified one with `simplified`);
    every feature gets `valid`, `crossings`, `overlaps` and `touches`.  `not_valid` (with `simplified`): ids that keep their raw
    vertices in every ring, as an object below `min_iou` does.
    `shared` (with `simplified` = the rings and vertices of `c3d_outlines_simplify_shared`): its `left` labels.  No ring ever
    falls back to its raw vertices then, since that would break the sharing: an object whose outline collapsed (fewer than 3
    vertices, or a doubled area that is zero or changed its sign) is written with "geometry": null, a hole that did is left out,
    and every feature gets `neighbours`, the sorted ids on the other side of its walls, and `collapsed`.
    `refined` (with `shared`, of `c3d_outlines_simplify_safe`) = (level [vertices], node [vertices]) of the simplified vertices:
    every feature gets `refined`, the number of its arcs -- which start at the node vertices of a ring, or at the first vertex of a
    ring without one -- whose level is above 0."""
    table, rings, vertices = np.asarray(table), np.asarray(rings), np.asarray(vertices)
    if simplified is not None:
        rings_s, vertices_s = np.asarray(simplified[0]).tolist(), np.asarray(simplified[1])
    by_id = {}
    for at, row in enumerate(rings.tolist()):
        by_id.setdefault(row[0], []).append(row + [at])
    features, skipped = [], []
    for k, (area, _, _, _, _, cls, _, score_q) in enumerate(table.tolist()):
        own = by_id.get(k + 1, [])
        outline = [r for r in own if r[3] > 0]
        if len(outline) != 1 or any(r[1] < 0 or r[1] + r[2] > len(vertices) for r in own) or sum(r[3] for r in own) != area:
            skipped.append(k + 1)
            continue
        coords, n_raw, n_out = [], 0, 0
        neighbours, collapsed, gone, n_refined = set(), False, False, 0
        drifted = simplified is not None and iou is not None and min_iou is not None and not float(iou[k]) > min_iou
        drifted = drifted or (simplified is not None and not_valid is not None and k + 1 in not_valid)
        for r in outline + [r for r in own if r[3] <= 0]:  # the outline, then the holes in ring order
            ring = vertices[r[1]:r[1] + r[2]].tolist()
            n_raw += len(ring)
            if shared is not None:
                s = rings_s[r[8]]
                if 0 <= s[1] and s[1] + s[2] <= len(vertices_s):      # also of a ring that collapsed: the wall is still shared
                    neighbours.update(int(v) for v in shared[s[1]:s[1] + s[2]] if v > 0)
                    if refined is not None and s[2] > 0:
                        up, node = refined[0][s[1]:s[1] + s[2]] > 0, refined[1][s[1]:s[1] + s[2]]
                        n_refined += int((up & node).sum()) if node.any() else int(up[0])
                if s[1] < 0 or s[1] + s[2] > len(vertices_s) or s[2] < 3 or s[3] == 0 or (s[3] > 0) != (r[3] > 0):
                    collapsed = True
                    gone = gone or r[3] > 0
                    continue
                ring = vertices_s[s[1]:s[1] + s[2]].tolist()
            elif simplified is not None and not drifted:
                s = rings_s[r[8]]
                if s[1] >= 0 and s[1] + s[2] <= len(vertices_s) and s[3] != 0 and (s[3] > 0) == (r[3] > 0):
                    ring = vertices_s[s[1]:s[1] + s[2]].tolist()
            n_out += len(ring)
            coords.append(ring + ring[:1])
        properties = {"id": k + 1, "area": area, "cls": cls, "score": round(score_q / 65535, 4), "perimeter": outline[0][4]}
        if simplified is not None:
            properties.update(vertices_raw=n_raw, vertices=n_out)
            if iou is not None:
                properties.update(iou=round(float(iou[k]), 4))
        if shared is not None:
            properties.update(neighbours=sorted(neighbours), collapsed=collapsed)
            if refined is not None:
                properties.update(refined=n_refined)
        if extra is not None:
            properties.update(extra.get(k + 1, {}))
        if validity is not None:
            properties.update(validity_properties(validity[k] if k < len(validity) else EMPTY_ROW))
        geometry = None if gone else {"type": "Polygon", "coordinates": coords}
        features.append({"type": "Feature", "geometry": geometry, "properties": properties})
    return {"type": "FeatureCollection", "features": features}, skipped


def add_validity(sums, stage, name, found):
    """Adds the counts of one `SceneValidity` to the run's sums of its stage and returns its rows [K, 8] on the host, K = the
    largest object id of the ring table.  An object that could not be checked (its rings were cut off, or its edge pairs
    exceed the work cap) is remembered as `<scene>:<id>` for the closing line."""
    checked, invalid, empty, incomplete, over, crossings, overlaps, _ = (int(v) for v in found.counts.cpu().tolist())
    objects = checked + empty + incomplete + over
    rows = found.valid[:objects].cpu().numpy()
    s = sums.setdefault(stage, dict(counts=dict(objects=0, checked=0, invalid=0, crossings=0, overlaps=0), unchecked=[]))
    for key, value in (("objects", objects), ("checked", checked), ("invalid", invalid), ("crossings", crossings), ("overlaps", overlaps)):
        s["counts"][key] += value
    s["unchecked"] += [f"{name}:{k + 1}" for k in np.nonzero(rows[:, 0])[0].tolist()]
    return rows


def conflict_properties(row):
    """The feature properties of one row of a `SceneConflicts`."""
    _, partner, _, cross, same, opposite, _, _ = (int(v) for v in row)
    return dict(conflicts=cross + same, conflict_with=partner, shared_walls=opposite)


def in_conflict_ids(rows):
    """The ids of the rows of a `SceneConflicts` (host array [rows, 8]) that were checked and cross or overlap another object."""
    return {k + 1 for k, row in enumerate(np.asarray(rows).tolist()) if row[0] == 0 and row[3] + row[4] > 0}


def read_conflicts(found):
    """(rows [K, 8] on the host, dict of the counts) of one `SceneConflicts`, K = the largest object id of the ring table."""
    checked, bad, empty, incomplete, over, crossings, overlaps, _ = (int(v) for v in found.counts.cpu().tolist())
    objects = checked + empty + incomplete + over
    counts = dict(objects=objects, checked=checked, in_conflict=bad, crossings=crossings, overlaps=overlaps,
                  shared_walls=int(found.info[6]))
    return found.conflict[:objects].cpu().numpy(), counts


def add_conflicts(sums, stage, name, rows, counts, rounds=None, remaining=()):
    """Adds the counts of one scene to the run's sums of its stage; an object that could not be checked is remembered as
    `<scene>:<id>`, and so is one that `--clean_rounds` left in conflict."""
    s = sums.setdefault(stage, dict(counts=dict.fromkeys(counts, 0), unchecked=[], rounds=None, remaining=[]))
    for key, value in counts.items():
        s["counts"][key] += value
    s["unchecked"] += [f"{name}:{k + 1}" for k in np.nonzero(rows[:, 0] > 1)[0].tolist()]
    if rounds is not None:
        s["rounds"] = max(s["rounds"] or 0, rounds)
        s["remaining"] += [f"{name}:{k}" for k in sorted(remaining)]


def doc_table(doc, frac_bits, device):
    """The ring table (rings i32 [., 8], vertices i32 [., 2], counts i32 [5]) of the polygons of a FeatureCollection as it is
    written, on `device`: one ring per linear ring without its closing vertex, coordinates times 2^frac_bits."""
    rows, verts = [], []
    for feature in doc["features"]:
        for ring in (feature["geometry"] or {"coordinates": []})["coordinates"]:
            rows.append([feature["properties"]["id"], len(verts), len(ring) - 1, 0, 0, 0, 0, 0])
            verts += [[int(round(x * (1 << frac_bits))), int(round(y * (1 << frac_bits)))] for x, y in ring[:-1]]
    rings = torch.tensor(rows or [[0] * 8], dtype=torch.int32, device=device).reshape(-1, 8)
    vertices = torch.tensor(verts or [[0, 0]], dtype=torch.int32, device=device).reshape(-1, 2)
    counts = torch.tensor([len(rows), len(rows), len(verts), len(verts), 0], dtype=torch.int32, device=device)
    return rings, vertices, counts


def clean_file(path, write, first_bad, frac_bits, max_rounds, max_objects, device):
    """The loop of `--simplify_clean` / `--regularize_clean` on one written file: `write(ids)` writes `path` with those ids on their
    fallback; the file is read back, uploaded as a ring table and checked (`ops.rings_conflicts`), and what is in conflict falls
    back, for at most `max_rounds` rounds.  Returns (rounds, the ids still in conflict, the last check or None)."""
    from ..infer import SceneConflicts
    bad, fallen, rounds, found = set(first_bad), set(), 0, None
    while rounds < max_rounds:
        fallen |= bad
        rounds += 1
        write(fallen)
        with open(path) as f:
            doc = json.load(f)
        found = SceneConflicts(*ops.rings_conflicts(*doc_table(doc, frac_bits, device), frac_bits=frac_bits, max_objects=max_objects))
        bad = in_conflict_ids(read_conflicts(found)[0])
        if not bad:
            break
    return rounds, bad, found


def add_conflict_properties(path, rows):
    """Rewrites the FeatureCollection at `path` with `conflicts`, `conflict_with` and `shared_walls` on every feature."""
    with open(path) as f:
        doc = json.load(f)
    for feature in doc["features"]:
        k = feature["properties"]["id"]
        feature["properties"].update(conflict_properties(rows[k - 1] if k - 1 < len(rows) else EMPTY_ROW))
    with open(path, "w") as f:
        json.dump(doc, f)


def simplify_ious(objects, fill):
    """(iou f64 [rows], kept, vanished) of a `SceneFill` against the raw `objects`: the IoU of every raw object with its partner
    among the filled simplified polygons, 0 without one; how many objects have their own id as partner; how many own no pixel
    after the fill."""
    rows = int(objects.counts[1])
    if int(fill.info[0]) & (L.FILL_ST_BAD_ID | L.FILL_ST_BAD_RING) or int(fill.match[3][4]):
        raise SystemExit(f"--simplify_check: c3d_rings_fill status {int(fill.info[0])}, c3d_objects_match status {int(fill.match[3][4])}")
    match = fill.match[0][:rows].cpu().numpy().astype(np.int64)
    iou = np.where(match[:, 2] > 0, match[:, 1] / np.maximum(match[:, 2], 1), 0.0)
    kept = int((match[:, 0] == np.arange(1, rows + 1)).sum())
    vanished = int((fill.table[:rows, 0].cpu().numpy() == 0).sum())
    return iou, kept, vanished


def node_vertices(objects, vertices):
    """bool [n] on the device: which of the lattice points `vertices` i32 [n, 2] = (vx, vy) are nodes of the label map of
    `objects`, by the rule of c3d_outlines_simplify_shared: the four labels round the point differ across three of its four
    sides or more."""
    rows = objects.counts[1].clamp(0, objects.table.shape[0])
    lab = torch.where((objects.labels >= 1) & (objects.labels <= rows), objects.labels, torch.zeros_like(objects.labels))
    lab = torch.nn.functional.pad(lab, (1, 1, 1, 1))          # l(y, x) is lab[y + 1, x + 1]
    vx, vy = vertices[:, 0].long(), vertices[:, 1].long()
    a, b, c, d = lab[vy, vx], lab[vy, vx + 1], lab[vy + 1, vx], lab[vy + 1, vx + 1]
    return (a != b).int() + (c != d).int() + (a != c).int() + (b != d).int() >= 3


def save_polygons(path, objects, outlines, simplified=None, iou=None, min_iou=None, extra=None, validity=None, not_valid=None):
    """objects/<name>.geojson; the one read-back of the rings (`simplified`: the second `SceneOutlines` of
    `predict(..., simplify=tol)`, read back with them; `iou`, `min_iou`: see `polygons_geojson`).  Returns the ids that were
    left out."""
    ring_rows, written = int(outlines.counts[1]), int(outlines.counts[3])
    rows = int(objects.counts[1])
    shared, refined = None, None
    if simplified is not None:
        if hasattr(simplified, "left"):                   # a SceneSharedOutlines of --simplify_shared
            shared = simplified.left[:int(simplified.counts[3])].cpu().numpy()
        if hasattr(simplified, "level"):                  # a SceneSafeOutlines of --simplify_safe
            n_out = int(simplified.counts[3])
            refined = (simplified.level[:n_out].cpu().numpy(), node_vertices(objects, simplified.vertices[:n_out]).cpu().numpy())
        simplified = (simplified.rings[:ring_rows].cpu().numpy(), simplified.vertices[:int(simplified.counts[3])].cpu().numpy())
    doc, skipped = polygons_geojson(objects.table[:rows].cpu().numpy(), outlines.rings[:ring_rows].cpu().numpy(),
                                    outlines.vertices[:written].cpu().numpy(), simplified, iou, min_iou, extra, validity, not_valid,
                                    shared, refined)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f)
    if skipped:
        print(f"{path}: {len(skipped)} of {rows} objects left out, their rings were cut off (status {int(outlines.counts[4])})")
    return skipped


def regular_geojson(doc, rings, regular, iou=None, min_iou=None, validity=None, not_valid=None):
    """(FeatureCollection dict, objects regularised, objects on their fallback) for objects/<name>.regular.geojson: the
    features and properties of `doc` (objects/<name>.geojson), each with `regular` and the coordinates of the regularised
    rings, sixteenths of a pixel as floats.  `rings` [ring rows, 8] are the raw rings, `regular` = (rings, vertices) of
    `c3d_rings_regularize`, row for row.  An object keeps the coordinates it has in `doc` and gets `regular: false` where one of
    its rings was copied or has no vertices, where the doubled area of a regularised ring is zero or has the other sign than
    the raw ring's, or where `iou` [rows] (its regularised polygon filled back, against its raw pixels; every feature gets it
    as `iou`) is not above `min_iou`, or where its id is in `not_valid`.  `validity` [rows, 8]: the rows of `c3d_rings_valid` on
    the regularised rings, which replace the `valid`, `crossings`, `overlaps` and `touches` of `doc`."""
    rings_q, vertices_q = np.asarray(regular[0]).tolist(), np.asarray(regular[1]).astype(np.int64)
    scale = float(1 << REGULAR_FRAC_BITS)
    by_id = {}
    for at, row in enumerate(np.asarray(rings).tolist()):
        by_id.setdefault(row[0], []).append(row + [at])
    features, done = [], 0
    for feature in doc["features"]:
        k = feature["properties"]["id"]
        own = by_id.get(k, [])
        coords, ok = [], not (iou is not None and min_iou is not None and not float(iou[k - 1]) > min_iou)
        ok = ok and not (not_valid is not None and k in not_valid)
        for r in [r for r in own if r[3] > 0] + [r for r in own if r[3] <= 0]:   # the order of polygons_geojson
            q = rings_q[r[8]]
            if not ok or q[3] != 1 or q[1] < 0 or q[1] + q[2] > len(vertices_q):
                ok = False
                break
            v = vertices_q[q[1]:q[1] + q[2]]
            area2 = int((np.roll(v[:, 0], 1) * v[:, 1] - v[:, 0] * np.roll(v[:, 1], 1)).sum())
            if area2 == 0 or (area2 > 0) != (r[3] > 0):
                ok = False
                break
            ring = (v / scale).tolist()
            coords.append(ring + ring[:1])
        ok = ok and feature["geometry"] is not None       # a collapsed outline of --simplify_shared: nothing to square or to keep
        properties = dict(feature["properties"], regular=ok)
        if iou is not None:
            properties["iou"] = round(float(iou[k - 1]), 4)
        if validity is not None:
            properties.update(validity_properties(validity[k - 1] if k - 1 < len(validity) else EMPTY_ROW))
        done += ok
        if feature["geometry"] is None:
            features.append({"type": "Feature", "geometry": None, "properties": properties})
            continue
        features.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": coords if ok else feature["geometry"]["coordinates"]},
                         "properties": properties})
    return {"type": "FeatureCollection", "features": features}, done, len(features) - done


def save_regular(path, main_path, outlines, regular, iou=None, min_iou=None, validity=None, not_valid=None):
    """objects/<name>.regular.geojson from objects/<name>.geojson, which was just written, and the read-back of a `SceneRegular`."""
    with open(main_path) as f:
        doc = json.load(f)
    ring_rows = int(outlines.counts[1])
    out, done, fallback = regular_geojson(doc, outlines.rings[:ring_rows].cpu().numpy(),
                                          (regular.rings[:ring_rows].cpu().numpy(), regular.vertices[:int(regular.counts[3])].cpu().numpy()),
                                          iou, min_iou, validity, not_valid)
    with open(path, "w") as f:
        json.dump(out, f)
    ids = [feat["properties"]["id"] for feat in out["features"]]
    return done, fallback, ids


def object_shapes(name, objects, shapes):
    """The read-back of a `SceneShapes`: (id -> shape properties, id -> closed hull ring, id -> closed rectangle ring) for the
    rows of the object table.  hull_area and rect_area are in square pixels, rect_long and rect_short in pixels, rect_angle
    is the direction of the long side in degrees in [0, 180), image coordinates; solidity and rectangularity divide the
    table's pixel area by them and are at most 1, because the pixels lie inside the hull of their corners."""
    status = int(shapes.counts[4])
    if status & (L.HULL_ST_BAD_ROW | L.HULL_ST_TRUNCATED):
        raise SystemExit(f"{name}: --shapes: c3d_rings_hull status {status}")
    rows, written = min(int(objects.counts[1]), int(shapes.counts[1])), int(shapes.counts[3])
    areas = objects.table[:rows, 0].cpu().tolist()
    hulls, rects = shapes.hulls[:rows].cpu().tolist(), shapes.rects[:rows].cpu().tolist()
    vertices = shapes.vertices[:written].cpu().tolist()
    props, hull_rings, rect_rings = {}, {}, {}
    for k, (h, r) in enumerate(zip(hulls, rects)):
        if h[1] < 0 or h[2] < 3 or r[0] < 0:             # an id without rings: its polygon is left out as well
            continue
        ring = vertices[h[1]:h[1] + h[2]]
        P, Q = ring[r[0]], ring[(r[0] + 1) % h[2]]
        corners, long_side, short_side, angle = ops.rect_corners(P, (Q[0] - P[0], Q[1] - P[1]), r)
        hull_area, rect_area = h[3] / 2, (r[3] - r[2]) * r[4] / r[1]
        props[k + 1] = dict(hull_area=hull_area, hull_vertices=h[2], solidity=round(areas[k] / hull_area, 4),
                            rect_area=round(rect_area, 4), rect_long=round(long_side, 4), rect_short=round(short_side, 4),
                            rect_angle=round(angle, 4), rectangularity=round(areas[k] / rect_area, 4))
        hull_rings[k + 1] = ring + ring[:1]
        rect_rings[k + 1] = corners.tolist() + corners[:1].tolist()
    return props, hull_rings, rect_rings


def save_shapes(path, objects, rings_by_id, skipped):
    """objects/<name>.hulls.geojson or .rects.geojson: one `Polygon` per object that has a feature in objects/<name>.geojson,
    with the CSV's id, area, cls and score."""
    table = objects.table[:int(objects.counts[1])].cpu().tolist()
    features = []
    for k, (area, _, _, _, _, cls, _, score_q) in enumerate(table):
        if k + 1 in rings_by_id and k + 1 not in skipped:
            features.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [rings_by_id[k + 1]]},
                             "properties": {"id": k + 1, "area": area, "cls": cls, "score": round(score_q / 65535, 4)}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)


LABEL_FRAC_BITS = 4                                       # polygon labels are rounded to 1/16 pixel


def polygon_labels(args, name, Hs, Ws, device):
    """The ground truth of `--label_polygons` for the scene `name`, filled on the device: labels, table, counts (what
    `ObjectEvaluator.update_labeled` takes), mask and cls_map u8 [Hs, Ws]."""
    path = args.label_polygons
    if os.path.isdir(path):
        found = [f for f in (os.path.join(path, name + ext) for ext in (".json", ".geojson")) if os.path.isfile(f)]
        if not found:
            raise SystemExit(f"--label_polygons: neither {name}.json nor {name}.geojson in {path}")
        path = found[0]
    try:
        rings, vertices, counts, id_cls = vector_labels.read_polygons(path, LABEL_FRAC_BITS)
    except (OSError, vector_labels.PolygonFileError) as e:
        raise SystemExit(f"--label_polygons: {e}")
    n = max(len(id_cls), 1)
    cls = np.zeros(n, dtype=np.uint8)
    cls[:len(id_cls)] = id_cls
    d_rings, d_vertices, d_counts = (torch.from_numpy(a).to(device) for a in (rings, vertices, counts))
    labels, table, counts_obj, mask, cls_map, info = ops.rings_fill(
        d_rings, d_vertices, d_counts, Hs, Ws, frac_bits=LABEL_FRAC_BITS,
        id_cls=torch.from_numpy(cls).to(device), max_objects=n, want_mask=True, want_cls_map=True)
    if int(info[0]):
        raise SystemExit(f"{path}: c3d_rings_fill status {int(info[0])}")
    return SimpleNamespace(labels=labels, table=table, counts=counts_obj, mask=mask, cls_map=cls_map, rings=d_rings, vertices=d_vertices,
                           ring_counts=d_counts)


def save_matches(path, objects, gt_counts, match_p, match_g):
    """objects/<name>.match.csv: the rows of the predicted objects, then those of the ground-truth objects under `# gt`."""
    rows_p, rows_g = int(objects.counts[1]), int(gt_counts[1])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("id,gt_id,inter,union,covered\n")
        for k, (partner, inter, union, covered) in enumerate(match_p[:rows_p].cpu().tolist()):
            f.write(f"{k + 1},{partner},{inter},{union},{covered}\n")
        f.write("# gt\nid,pred_id,inter,union,covered\n")
        for k, (partner, inter, union, covered) in enumerate(match_g[:rows_g].cpu().tolist()):
            f.write(f"{k + 1},{partner},{inter},{union},{covered}\n")


def print_object_scores(evaluator, per_class=False):
    s = evaluator.scores()
    line = (f"objects: tp = {s['tp']} fp = {s['fp']} fn = {s['fn']} precision = {s['precision']:.4f} recall = {s['recall']:.4f} "
            f"f1 = {s['f1']:.4f} sq = {s['sq']:.4f} rq = {s['rq']:.4f} pq = {s['pq']:.4f}")
    if per_class:
        line += f" class_f1 = [{', '.join(f'{v:.4f}' for v in s['class_f1'])}]"
    print(line)
    return s


def print_bda_scores(evaluator, object_hist, num_class):
    """The log columns of train_BDA.py's val; then the damage scores of the per-building majority map, where asked for."""
    loc_f1, harmonic, oaf1, damage_f1 = evaluator.scores()
    print(f"\nTest:\tloc_f1_score = {loc_f1:.4f}\tharmonic_mean_f1 = {harmonic:.4f}\toaf1 = {oaf1:.4f}\t"
          f"damage_f1_score = [{', '.join(f'{v:.4f}' for v in damage_f1)}]")
    if object_hist is None:
        return loc_f1, harmonic, oaf1, damage_f1
    per_object = Evaluator(num_class)                      # confusion_matrix[gt, pred]; c3d_hist2d counted [pred, gt]
    per_object.confusion_matrix = object_hist.matrix().T.astype(np.longlong)
    f1 = per_object.Damage_F1_socore()
    print(f"Objects:\tharmonic_mean_f1 = {len(f1) / np.sum(1.0 / f1):.4f}\tdamage_f1_score = [{', '.join(f'{v:.4f}' for v in f1)}]")
    return loc_f1, harmonic, oaf1, damage_f1


def save_polygon_scores(path, rows, results):
    """objects/<name>.polis.csv: per stage the rows of the predicted objects; `results` = (stage, pair, pair_n) device tensors."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("stage,id,gt_id,n,n_gt,polis,hausdorff,flag\n")
        for stage, pair, pair_n in results:
            for k, ((polis, hausdorff, _, _), (g, n_p, n_g, flag)) in enumerate(zip(pair[:rows].cpu().tolist(), pair_n[:rows].cpu().tolist())):
                f.write(f"{stage},{k + 1},{g},{n_p},{n_g},{polis:.4f},{hausdorff:.4f},{flag}\n")


def print_polygon_scores(evaluators):
    out = {}
    for stage, evaluator in evaluators.items():
        s = out[stage] = evaluator.scores()
        print(f"polygons[{stage}]: pairs = {s['pairs']} polis = {s['polis']:.4f} hausdorff_mean = {s['hausdorff_mean']:.4f} "
              f"hausdorff_max = {s['hausdorff_max']:.4f} n_ratio = {s['n_ratio']:.4f} skipped = {s['incomplete'] + s['over_work']}")
    return out


def print_boundary_scores(evaluator):
    s = evaluator.scores()
    print(f"boundary: d = {evaluator.d:g} tol = {evaluator.tau:g} biou = {s['boundary_iou']:.4f} precision = {s['boundary_precision']:.4f} "
          f"recall = {s['boundary_recall']:.4f} f1 = {s['boundary_f1']:.4f}")
    return s


def boundary_radius(text):
    v = float(text)
    if not 1.0 <= v <= 1024.0:                            # below 1 pixel a band or a tolerance holds no pixel of the lattice
        raise ArgumentTypeError(f"the radius must lie in [1, 1024] pixels, got {text}")
    return v


def split_rounds(text):
    v = int(text)
    if not 1 <= v <= 65536:
        raise ArgumentTypeError(f"--split_rounds must lie in [1, 65536], got {text}")
    return v


def check_split(name, objects):
    """Ends the run when the growth of `--split_objects` did not reach its fixed point on this scene."""
    info = getattr(objects, "info", None)
    if hasattr(objects, "key_map"):                       # the regions of --regions: their info is the sieve's (check_sieve)
        return
    if info is not None and int(info[0]) & L.SPLIT_ST_NOT_CONVERGED:
        raise SystemExit(f"{name}: the pieces of --split_objects were still growing after {int(info[2])} rounds; raise --split_rounds")


def sieve_area(text):
    v = int(text)
    if not 1 <= v <= 2 ** 20:
        raise ArgumentTypeError(f"--sieve must lie in [1, 2^20] pixels, got {text}")
    return v


def sieve_rounds(text):
    v = int(text)
    if not 1 <= v <= 65536:
        raise ArgumentTypeError(f"--sieve_rounds must lie in [1, 65536], got {text}")
    return v


def check_sieve(name, objects, rounds):
    """Ends the run when the sieve of `--sieve` stopped short on this scene."""
    status = int(objects.info[0])
    if status & L.SIEVE_ST_TABLE_FULL:
        Hs, Ws = objects.labels.shape
        raise SystemExit(f"{name}: --sieve: the border table of c3d_regions_sieve overflowed at its capacity of "
                         f"{ops.regions_sieve_plan(Hs, Ws)[1]} slots")
    if status & L.SIEVE_ST_NOT_CONVERGED:
        raise SystemExit(f"{name}: --sieve: small regions were still moving after {int(objects.info[1])} rounds; raise --sieve_rounds "
                         f"(now {rounds})")
    if status:
        raise SystemExit(f"{name}: --sieve: c3d_regions_sieve status {status}")


def add_region_properties(path, regions, num_class):
    """`from` and `to` on every feature of a .geojson of this run, decoded from its `cls` (the region's key)."""
    with open(path) as f:
        doc = json.load(f)
    for feature in doc["features"]:
        a, b = region_classes(feature["properties"]["cls"], regions, num_class)
        feature["properties"].update({"from": a, "to": b})
    with open(path, "w") as f:
        json.dump(doc, f)


def region_key_map(pre, post, change, regions, num_class):
    """The key map of `--regions` from label maps on the device, as `SceneInferencer.predict(regions=..)` keys the prediction."""
    pre, post = pre * change, post * change
    key = pre * num_class + post if regions == "transition" else (pre if regions == "pre" else post)
    return key.to(torch.uint8).contiguous()


def iou_threshold(text):
    v = float(text)
    if not 0.5 <= v < 1.0:
        raise ArgumentTypeError(f"--iou_thr must lie in [0.5, 1), got {text}")
    return v


def unit_interval(text):
    v = float(text)
    if not 0.0 <= v <= 1.0:
        raise ArgumentTypeError(f"the IoU bound must lie in [0, 1], got {text}")
    return v


def simplify_tolerance(text):
    v = float(text)
    if not 0.0 <= v <= 1024.0:
        raise ArgumentTypeError(f"the tolerance must lie in [0, 1024] pixels, got {text}")
    return v


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.polygons and not args.objects:
        parser.error("--polygons outlines the objects of the map: it needs --objects")
    if args.simplify is not None and not args.polygons:
        parser.error("--simplify simplifies the polygons: it needs --polygons")
    if args.shapes and not args.polygons:
        parser.error("--shapes describes the polygons: it needs --polygons")
    if args.simplify_min_iou is not None:
        args.simplify_check = True
    if args.simplify_check and args.simplify is None:
        parser.error("--simplify_check and --simplify_min_iou measure what --simplify cost: they need --simplify")
    if args.safe_rounds is not None and not args.simplify_safe:
        parser.error("--safe_rounds limits the rounds of --simplify_safe: it needs --simplify_safe")
    if args.simplify_safe:
        args.simplify_shared = True
        args.safe_rounds = 8 if args.safe_rounds is None else args.safe_rounds
        if not 1 <= args.safe_rounds <= 64:
            parser.error(f"--safe_rounds must lie in [1, 64], got {args.safe_rounds}")
    if args.simplify_shared and args.simplify is None:
        parser.error("--simplify_shared chooses how --simplify simplifies: it needs --simplify")
    if args.simplify_shared and (args.simplify_min_iou is not None or args.simplify_valid or args.simplify_clean):
        parser.error("--simplify_shared shares every wall between its two objects: a fall-back of single objects to their raw vertices "
                     "(--simplify_min_iou, --simplify_valid, --simplify_clean) would break that")
    if args.regularize_min_iou is not None and not args.regularize:
        parser.error("--regularize_min_iou is the fallback threshold of --regularize: it needs --regularize")
    if args.regularize and (not args.polygons or args.simplify is None):
        parser.error("--regularize squares the simplified polygons: it needs --polygons --simplify TOL")
    if args.simplify_valid and args.simplify is None:
        parser.error("--simplify_valid is a fallback of --simplify: it needs --simplify")
    if args.regularize_valid and not args.regularize:
        parser.error("--regularize_valid is a fallback of --regularize: it needs --regularize")
    if args.simplify_valid or args.regularize_valid:
        args.validity = True
    if args.validity and not args.polygons:
        parser.error("--validity tests the polygons: it needs --polygons")
    if args.simplify_clean and args.simplify is None:
        parser.error("--simplify_clean is a fallback of --simplify: it needs --simplify")
    if args.regularize_clean and not args.regularize:
        parser.error("--regularize_clean is a fallback of --regularize: it needs --regularize")
    if args.simplify_clean or args.regularize_clean:
        args.conflicts = True
    if args.conflicts and not args.polygons:
        parser.error("--conflicts compares the polygons: it needs --polygons")
    if args.clean_rounds < 0:
        parser.error("--clean_rounds must not be negative")
    if args.label_polygons and args.task == "SCD":
        parser.error("--label_polygons gives objects with one class each: it serves --task BCD and BDA")
    if args.label_polygons and any((args.label, args.label1, args.label2, args.change)):
        parser.error("--label_polygons replaces the label rasters: give one or the other")
    if args.boundary_tol is not None and args.boundary is None:
        parser.error("--boundary_tol is the tolerance of the boundary scores: it needs --boundary")
    if args.split_objects is not None and not args.objects:
        parser.error("--split_objects splits the objects of the map: it needs --objects")
    if args.split_rounds is not None and args.split_objects is None:
        parser.error("--split_rounds is the round limit of --split_objects: it needs --split_objects")
    if args.regions is not None:
        if args.task != "SCD":
            parser.error("--regions labels the class maps of --task SCD")
        if not args.objects:
            parser.error("--regions chooses what --objects labels: it needs --objects")
        if args.split_objects is not None:
            parser.error("--regions and --split_objects both replace the labelling: give one of them")
        if args.regions == "transition" and num_classes(args) > 16:
            parser.error("--regions transition keys a region by from * num_class + to in a byte: it serves at most 16 classes")
    if args.sieve is not None and args.regions is None:
        parser.error("--sieve absorbs the small regions of --regions: it needs --regions")
    if args.sieve_rounds is not None and args.sieve is None:
        parser.error("--sieve_rounds is the round limit of --sieve: it needs --sieve")
    if args.polygon_scores and not (args.label_polygons and args.polygons):
        parser.error("--polygon_scores compares the polygons of the map with labelled ones: it needs --label_polygons and --objects --polygons")
    return args


def main(argv=None):
    args = parse_args(argv)
    num_class = num_classes(args)
    if not args.file_root and not (args.pre and args.post):
        raise SystemExit("give --pre and --post, or --file_root")
    device = torch.device("cuda", args.gpu_id)
    torch.cuda.set_device(device)
    model = build_model(args, device)
    inf = SceneInferencer(model, args.task.lower(), stride=args.stride, window=args.window, batch=args.batch_size,
                          tta=None if args.tta == "none" else args.tta)
    meter = {"BCD": lambda: ConfuseMatrixMeter(n_class=2), "SCD": lambda: SCDHistogram(num_class, device),
             "BDA": lambda: BDAEvaluator(num_class, device)}[args.task]()
    object_hist = SCDHistogram(num_class, device) if args.task == "BDA" and args.objects else None
    object_eval = None                                    # made by the first labelled scene of a run with --objects
    boundary_eval = None                                  # made by the first labelled scene of a run with --boundary
    polygon_evals = {}                                    # --polygon_scores: stage -> PolygonEvaluator, in the order of the stages
    scored = 0
    cut_off = 0                                           # objects whose polygon was left out of a .geojson

    def score_objects(name, objects, gt_mask, gt_cls=None, gt=None):
        nonlocal object_eval
        if object_eval is None:
            object_eval = ObjectEvaluator(n_cls=1 if args.regions == "transition" else num_class, iou_thr=args.iou_thr,
                                          connectivity=args.connectivity, device=device)
        if gt is not None:                                # polygon labels are objects already: no relabelling
            match_p, match_g = object_eval.update_labeled(objects, gt.labels, gt.table, gt.counts)
        else:
            match_p, match_g = object_eval.update(objects, gt_mask.to(torch.uint8), None if gt_cls is None else gt_cls.to(torch.uint8))
        save_matches(os.path.join(args.out_dir, "objects", name + ".match.csv"), objects, object_eval.last_gt_counts, match_p, match_g)
        return match_p

    def score_polygons(name, objects, stages, gt, match_p):
        results = []
        for stage, rings, frac_bits in stages:            # each a SceneOutlines or SceneRegular of this scene
            if stage not in polygon_evals:
                polygon_evals[stage] = PolygonEvaluator(device=device)
            pair, pair_n, _, _ = polygon_evals[stage].update(rings.rings, rings.vertices, rings.counts, frac_bits, gt.rings, gt.vertices,
                                                             gt.ring_counts, LABEL_FRAC_BITS, match_p, gt.table.shape[0])
            results.append((stage, pair, pair_n))
        save_polygon_scores(os.path.join(args.out_dir, "objects", name + ".polis.csv"), int(objects.counts[1]), results)

    def score_boundary(mask, gt_mask):
        nonlocal boundary_eval
        if args.boundary is None:
            return
        if boundary_eval is None:
            boundary_eval = BoundaryEvaluator(args.boundary, args.boundary_tol, device=device)
        boundary_eval.update(mask.to(torch.uint8), gt_mask.to(torch.uint8))

    split = {} if args.split_objects is None else dict(split=args.split_objects, split_rounds=args.split_rounds)
    if args.regions is not None:
        split.update(regions=args.regions, sieve=args.sieve, sieve_rounds=args.sieve_rounds)
    region_sums = dict(objects=0, moved=0, pixels=0, rounds=0)                   # --regions over all scenes
    if args.simplify_check:
        split["simplify_check"] = True
    if args.simplify_shared:
        split["simplify_shared"] = True
    if args.simplify_safe:
        split.update(simplify_safe=True, safe_rounds=args.safe_rounds)
    if args.shapes:
        split["shapes"] = True
    if args.regularize:
        split["regularize"] = True
        split["regularize_check"] = args.regularize_min_iou is not None
    if args.validity:
        split["validity"] = True
    if args.conflicts:
        split["conflicts"] = True
    shared_sums = dict(objects=0, nodes=0, arcs=0, shared_arcs=0, collapsed=0)   # --simplify_shared over all scenes
    safe_sums = dict(rounds=0, raised=0, refined=0, raw=0, first=0, last=0)      # --simplify_safe over all scenes
    conflict_sums = {}                                    # --conflicts over all scenes: stage -> counts, objects by name
    validity_sums = {}                                    # --validity over all scenes: stage -> counts, unchecked objects by name
    squared =dict(objects=0, regular=0, fallback=0, iou_sum=0.0, iou_min=1.0)   # --regularize over all scenes
    drift = dict(objects=0, kept=0, vanished=0, iou_sum=0.0, iou_min=1.0)   # --simplify_check over all scenes
    shape_sums = dict(objects=0, solidity=0.0, rectangularity=0.0)          # --shapes over all scenes
    for name, img, label in scenes(args):
        scene = torch.from_numpy(np.ascontiguousarray(img))
        gt = polygon_labels(args, name, img.shape[0], img.shape[1], device) if args.label_polygons else None
        if args.polygons:                 # the outlines come last; every `out[-1]` below is the objects
            out = inf.predict(scene, objects=True, min_area=args.min_area, connectivity=args.connectivity, outlines=True,
                              max_rings=args.max_rings, max_vertices=args.max_vertices, simplify=args.simplify, **split)
            simplified, iou, shapes, regular, regular_iou = None, None, None, None, None
            conf = {}                         # stage -> (host rows, counts) of its `SceneConflicts`
            if args.conflicts:            # appended after the validity entries, in the same order
                stages_c = ["raw"] + (["simplified"] if args.simplify is not None else []) + (["regular"] if args.regularize else [])
                out, found_c = out[:-len(stages_c)], out[-len(stages_c):]
                conf = {stage: read_conflicts(v) for stage, v in zip(stages_c, found_c)}
            valid_rows = {}                   # stage -> host rows of its `SceneValidity`
            if args.validity:             # appended last of all: raw, then simplified, then regularised
                stages_v = ["raw"] + (["simplified"] if args.simplify is not None else []) + (["regular"] if args.regularize else [])
                out, found_v = out[:-len(stages_v)], out[-len(stages_v):]
                for stage, v in zip(stages_v, found_v):
                    valid_rows[stage] = add_validity(validity_sums, stage, name, v)
            if args.regularize:         # appended last: the regularised rings, then their check
                if args.regularize_min_iou is not None:
                    out, regular_fill = out[:-1], out[-1]
                out, regular = out[:-1], out[-1]
            if args.shapes:               # appended after the simplified rings and their check
                out, shapes = out[:-1], out[-1]
            if args.simplify_check:
                out, fill = out[:-1], out[-1]
                iou, kept, vanished = simplify_ious(out[-3], fill)
                drift = dict(objects=drift["objects"] + len(iou), kept=drift["kept"] + kept, vanished=drift["vanished"] + vanished,
                             iou_sum=drift["iou_sum"] + float(iou.sum()), iou_min=min([drift["iou_min"]] + iou.tolist()))
            if args.simplify is not None:
                out, simplified = out[:-1], out[-1]
            if args.simplify_shared:
                if int(simplified.counts[4]) & (L.OUTLINE_ST_BAD_COUNTS | L.SIMPLIFY_ST_BAD_INPUT):
                    raise SystemExit(f"{name}: --simplify_shared: c3d_outlines_simplify_shared status {int(simplified.counts[4])}")
                _, nodes, arcs, _, shared_arcs, collapsed, _, _ = (int(v) for v in simplified.info.cpu().tolist())
                shared_sums = dict(objects=shared_sums["objects"] + int(out[-2].counts[1]), nodes=shared_sums["nodes"] + nodes,
                                   arcs=shared_sums["arcs"] + arcs, shared_arcs=shared_sums["shared_arcs"] + shared_arcs,
                                   collapsed=shared_sums["collapsed"] + collapsed)
            if args.simplify_safe:
                rounds, raised, refined, at_cap, first, last, _, status = (int(v) for v in simplified.safe.cpu().tolist())
                if status == 3:
                    raise SystemExit(f"{name}: --simplify_safe: the edge grid of round {rounds - 1} is above the work cap of "
                                     f"c3d_outlines_simplify_safe (work {int(simplified.info[7])}): the outlines were not checked")
                if status == 2:
                    raise SystemExit(f"{name}: --simplify_safe: {last} defective pairs are left after {rounds} rounds and no arc can be "
                                     f"refined further: the rings do not belong to the label map, and more rounds cannot help")
                if status != 0:
                    raise SystemExit(f"{name}: --simplify_safe did not converge in {rounds} rounds ({last} defective pairs left, status "
                                     f"{status}): raise --safe_rounds (now {args.safe_rounds})")
                safe_sums = dict(rounds=max(safe_sums["rounds"], rounds), raised=max(safe_sums["raised"], raised),
                                 refined=safe_sums["refined"] + refined, raw=safe_sums["raw"] + at_cap, first=safe_sums["first"] + first,
                                 last=safe_sums["last"] + last)
            check_split(name, out[-2])
            written_v = valid_rows.get("simplified" if simplified is not None else "raw")   # of the coordinates that are written
            bad_v = not_valid_ids(valid_rows["simplified"]) if args.simplify_valid else None
            main_path = os.path.join(args.out_dir, "objects", name + ".geojson")
            if shapes is None:
                cut_off += len(save_polygons(main_path, out[-2], out[-1], simplified, iou, args.simplify_min_iou, None, written_v, bad_v))
            else:
                props, hull_rings, rect_rings = object_shapes(name, out[-2], shapes)
                skipped = save_polygons(os.path.join(args.out_dir, "objects", name + ".geojson"), out[-2], out[-1], simplified, iou,
                                        args.simplify_min_iou, props, written_v, bad_v)
                cut_off += len(skipped)
                save_shapes(os.path.join(args.out_dir, "objects", name + ".hulls.geojson"), out[-2], hull_rings, set(skipped))
                save_shapes(os.path.join(args.out_dir, "objects", name + ".rects.geojson"), out[-2], rect_rings, set(skipped))
                kept = [v for k, v in props.items() if k not in set(skipped)]
                shape_sums = dict(objects=shape_sums["objects"] + len(kept),
                                  solidity=shape_sums["solidity"] + sum(v["solidity"] for v in kept),
                                  rectangularity=shape_sums["rectangularity"] + sum(v["rectangularity"] for v in kept))
            most = max(int(out[-2].counts[1]), 1)
            if args.conflicts:            # the main file: fall back and check again, then the properties of what is written
                written_stage = "simplified" if simplified is not None else "raw"
                rows_c, counts_c = conf[written_stage]
                rounds, left = None, ()
                if args.simplify_clean:
                    rounds, left, last = clean_file(
                        main_path, lambda ids: save_polygons(main_path, out[-2], out[-1], simplified, iou, args.simplify_min_iou,
                                                             props if shapes is not None else None, written_v, set(bad_v or ()) | ids),
                        in_conflict_ids(rows_c), 0, args.clean_rounds, most, device)
                    if last is not None:
                        rows_c, counts_c = read_conflicts(last)
                add_conflict_properties(main_path, rows_c)
                for stage, (rows_s, counts_s) in conf.items():
                    if stage == written_stage:
                        add_conflicts(conflict_sums, stage, name, rows_c, counts_c, rounds, left)
                    elif stage != "regular":
                        add_conflicts(conflict_sums, stage, name, rows_s, counts_s)
            if regular is not None:
                if int(regular.counts[4]) & (L.OUTLINE_ST_BAD_COUNTS | L.REGULAR_ST_BAD_ROW):
                    raise SystemExit(f"{name}: --regularize: c3d_rings_regularize status {int(regular.counts[4])}")
                if args.regularize_min_iou is not None:
                    regular_iou = simplify_ious(out[-2], regular_fill)[0]
                regular_path = os.path.join(args.out_dir, "objects", name + ".regular.geojson")
                bad_r = not_valid_ids(valid_rows["regular"]) if args.regularize_valid else None
                done, fallback, ids = save_regular(regular_path, main_path, out[-1], regular, regular_iou, args.regularize_min_iou,
                                                   valid_rows.get("regular"), bad_r)
                if args.conflicts:
                    rows_c, counts_c = conf["regular"]
                    rounds, left, kept = None, (), [(done, fallback, ids)]
                    if args.regularize_clean:
                        rounds, left, last = clean_file(
                            regular_path, lambda bad: kept.append(save_regular(regular_path, main_path, out[-1], regular, regular_iou,
                                                                               args.regularize_min_iou, valid_rows.get("regular"),
                                                                               set(bad_r or ()) | bad)),
                            in_conflict_ids(rows_c), REGULAR_FRAC_BITS, args.clean_rounds, most, device)
                        done, fallback, ids = kept[-1]
                        if last is not None:
                            rows_c, counts_c = read_conflicts(last)
                    add_conflict_properties(regular_path, rows_c)
                    add_conflicts(conflict_sums, "regular", name, rows_c, counts_c, rounds, left)
                ious = [float(regular_iou[k - 1]) for k in ids] if regular_iou is not None else []
                squared = dict(objects=squared["objects"] + len(ids), regular=squared["regular"] + done,
                               fallback=squared["fallback"] + fallback, iou_sum=squared["iou_sum"] + sum(ious),
                               iou_min=min([squared["iou_min"]] + ious))
            if args.regions is not None:  # after every rewrite of the files above
                written = [main_path] + ([regular_path] if regular is not None else []) + \
                          ([main_path[:-len(".geojson")] + ext for ext in (".hulls.geojson", ".rects.geojson")] if shapes is not None else [])
                for path in written:
                    add_region_properties(path, args.regions, num_class)
            if args.polygon_scores:
                stages = [("raw", out[-1], 0)] + ([("simplified", simplified, 0)] if simplified is not None else []) + \
                         ([("regularised", regular, REGULAR_FRAC_BITS)] if regular is not None else [])
            out = out[:-1]
        elif args.objects:
            out = inf.predict(scene, objects=True, min_area=args.min_area, connectivity=args.connectivity, **split)
            check_split(name, out[-1])
        else:
            out = inf.predict(scene)
        if args.task == "BCD":
            mask = out[1]
            save_png(os.path.join(args.out_dir, name + ".png"), mask.cpu().numpy() * 255)
            if args.objects:
                save_objects(os.path.join(args.out_dir, "objects", name + ".csv"), out[-1])
            if gt is not None or label is not None:   # ceil(u8 / 255), the label side of c3d_bcd_preprocess
                lab = gt.mask > 0 if gt is not None else torch.from_numpy(np.ascontiguousarray(label)).to(device) > 0
                meter.update_cm_device(mask.float(), lab.float())
                if args.objects:
                    match_p = score_objects(name, out[-1], lab, gt=gt)
                    if args.polygon_scores:
                        score_polygons(name, out[-1], stages, gt, match_p)
                score_boundary(mask, lab)
                scored += 1
        elif args.task == "BDA":
            loc_prob, loc_mask, damage_map, cls_logits = out[:4]
            save_png(os.path.join(args.out_dir, "loc", name + ".png"), loc_mask.cpu().numpy() * 255)
            save_png(os.path.join(args.out_dir, "damage", name + ".png"), damage_map.cpu().numpy())
            if args.objects:
                save_png(os.path.join(args.out_dir, "damage_objects", name + ".png"), out[-1].object_cls.cpu().numpy())
                save_objects(os.path.join(args.out_dir, "objects", name + ".csv"), out[-1])
            if gt is not None or label is not None:   # scripts/train_BDA.py: label[:, 0].float() and the product of the two channels
                if gt is not None:       # the filled polygons: building mask and one damage class per building
                    loc, label_cls = gt.mask, gt.cls_map.long()
                else:
                    lab = torch.from_numpy(np.ascontiguousarray(label)).to(device)
                    loc, label_cls = lab[..., 0], lab[..., 0].long() * lab[..., 1].long()
                label_loc = loc.float()
                meter.add_batch(cls_logits[None], loc_prob[None, None], label_loc[None], label_cls[None])
                if args.objects:         # the per-building majority map against the damage labels, where there is one
                    inside = label_cls > 0
                    object_hist.update(out[-1].object_cls[inside], label_cls[inside])
                    match_p = score_objects(name, out[-1], loc > 0, label_cls, gt=gt)
                    if args.polygon_scores:
                        score_polygons(name, out[-1], stages, gt, match_p)
                score_boundary(loc_mask, loc > 0)
                scored += 1
        else:
            for sub, m in zip(("pred1", "pred2", "change"), out[:3]):
                save_png(os.path.join(args.out_dir, sub, name + ".png"), m.cpu().numpy() * (255 if sub == "change" else 1))
            if args.regions is not None:  # the regions of a class map; cls: the key.  The map that was vectorised goes out too
                found = out[-1]
                if args.sieve is not None:
                    check_sieve(name, found, args.sieve_rounds or 8)
                save_objects(os.path.join(args.out_dir, "objects", name + ".csv"), found, args.regions, num_class)
                key_map = found.key_map.cpu().numpy()
                if args.regions == "transition":
                    for side, m in zip(("from", "to"), region_classes(key_map, args.regions, num_class)):
                        save_png(os.path.join(args.out_dir, "regions", f"{name}.{side}.png"), m)
                else:
                    save_png(os.path.join(args.out_dir, "regions", name + ".png"), key_map)
                info = found.info.cpu().tolist()
                region_sums = dict(objects=region_sums["objects"] + int(found.counts[1]), moved=region_sums["moved"] + info[2],
                                   pixels=region_sums["pixels"] + info[3], rounds=max(region_sums["rounds"], info[1]))
            elif args.objects:           # the objects of the change mask; cls: the majority class of pred2 inside
                save_objects(os.path.join(args.out_dir, "objects", name + ".csv"), out[-1])
            if label is not None:        # reference scripts/train_SCD.py:216-217: the class labels count inside the change only
                lab = torch.from_numpy(np.ascontiguousarray(label)).to(device).long()
                meter.update(out[0], lab[..., 0] * lab[..., 2])
                meter.update(out[1], lab[..., 1] * lab[..., 2])
                if args.regions is not None:   # the regions of the label maps in the same mode, not sieved
                    gt_key = region_key_map(lab[..., 0], lab[..., 1], (lab[..., 2] > 0).long(), args.regions, num_class)
                    g_labels, g_table, _, _, g_counts = ops.scene_regions(gt_key, connectivity=args.connectivity, want_object_key=False)
                    score_objects(name, out[-1], None, gt=SimpleNamespace(labels=g_labels, table=g_table, counts=g_counts))
                elif args.objects:       # the objects of the change label; cls: the majority class of label2 inside
                    score_objects(name, out[-1], lab[..., 2] > 0, lab[..., 1])
                score_boundary(out[2], lab[..., 2] > 0)
                scored += 1
        print(f"{name}: {img.shape[0]} x {img.shape[1]} -> {args.out_dir}")
    if args.simplify_check:
        print(f"simplify: tol = {args.simplify:g} objects = {drift['objects']} kept = {drift['kept']} vanished = {drift['vanished']} "
              f"iou_mean = {drift['iou_sum'] / max(drift['objects'], 1):.4f} iou_min = {drift['iou_min'] if drift['objects'] else 0.0:.4f}")
    if args.simplify_shared:
        print(f"shared: tol = {args.simplify:g} objects = {shared_sums['objects']} nodes = {shared_sums['nodes']} "
              f"arcs = {shared_sums['arcs']} shared_arcs = {shared_sums['shared_arcs']} collapsed = {shared_sums['collapsed']}")
    if args.simplify_safe:
        print(f"safe: tol = {args.simplify:g} rounds = {safe_sums['rounds']} raised = {safe_sums['raised']} "
              f"arcs_refined = {safe_sums['refined']} arcs_raw = {safe_sums['raw']} defects = {safe_sums['first']} -> {safe_sums['last']}")
    if args.regions is not None:
        print(f"regions: mode = {args.regions} objects = {region_sums['objects']} moved = {region_sums['moved']} "
              f"pixels = {region_sums['pixels']} rounds = {region_sums['rounds']}")
    if args.shapes:
        n_shapes = max(shape_sums["objects"], 1)
        print(f"shapes: objects = {shape_sums['objects']} solidity_mean = {shape_sums['solidity'] / n_shapes:.4f} "
              f"rectangularity_mean = {shape_sums['rectangularity'] / n_shapes:.4f}")
    if args.regularize:
        checked = args.regularize_min_iou is not None and squared["objects"]
        print(f"regularize: objects = {squared['objects']} regular = {squared['regular']} fallback = {squared['fallback']} "
              f"iou_mean = {squared['iou_sum'] / max(squared['objects'], 1) if checked else 0.0:.4f} "
              f"iou_min = {squared['iou_min'] if checked else 0.0:.4f}")
    for stage, v in validity_sums.items():
        c = v["counts"]
        print(f"validity[{stage}]: objects = {c['objects']} valid = {c['checked'] - c['invalid']} invalid = {c['invalid']} "
              f"unchecked = {c['objects'] - c['checked']} crossings = {c['crossings']} overlaps = {c['overlaps']}" +
              (f" (unchecked: {', '.join(v['unchecked'])})" if v["unchecked"] else ""))
    for stage, v in conflict_sums.items():
        c = v["counts"]
        print(f"conflicts[{stage}]: objects = {c['objects']} clean = {c['checked'] - c['in_conflict']} in_conflict = {c['in_conflict']} "
              f"unchecked = {c['objects'] - c['checked']} crossings = {c['crossings']} overlaps = {c['overlaps']} "
              f"shared_walls = {c['shared_walls']}" +
              (f" rounds = {v['rounds']} remaining = {len(v['remaining'])}" if v["rounds"] is not None else "") +
              (f" (unchecked: {', '.join(v['unchecked'])})" if v["unchecked"] else ""))
    still = [n for v in conflict_sums.values() for n in v["remaining"]]
    if still:
        raise SystemExit(f"{len(still)} objects are still in conflict after --clean_rounds {args.clean_rounds}: {', '.join(still)}; "
                         f"raise --clean_rounds")
    if cut_off:
        raise SystemExit(f"{cut_off} objects have no polygon: their rings did not fit; raise --max_rings / --max_vertices")
    if not scored:
        return None
    if args.task == "BDA":
        result = print_bda_scores(meter, object_hist, num_class)
    elif args.task == "BCD":
        result = meter.get_scores()
        print(f"\nTest:\t Kappa (te) = {result['Kappa']:.4f}\t IoU (te) = {result['IoU']:.4f}\tF1 (te) = {result['F1']:.4f}\t "
              f"R (te) = {result['recall']:.4f}\tP (te) = {result['precision']:.4f}")
    else:
        result = meter.scores()
        print(f"Fscd: {result[0] * 100:.2f} IoU: {result[1] * 100:.2f} Sek: {result[2] * 100:.2f}")
    if object_eval is not None:
        print_object_scores(object_eval, per_class=args.task == "BDA" or args.regions in ("pre", "post"))
    if boundary_eval is not None:
        print_boundary_scores(boundary_eval)
    if polygon_evals:
        print_polygon_scores(polygon_evals)
    return result


def build_parser():
    p = ArgumentParser()
    p.add_argument("--task", choices=["BCD", "SCD", "BDA"], default="BCD")
    p.add_argument("--weights", required=True, help="best_model.pth (a state dict) or checkpoint.pth.tar of the training scripts")
    p.add_argument("--pre", default="")
    p.add_argument("--post", default="")
    p.add_argument("--label", default="", help="BCD change mask of the --pre / --post pair, scored when given")
    p.add_argument("--label1", default="", help="SCD: pre class map; scored when --label1, --label2 and --change are given.  BDA: "
                   "localisation (--label1) and damage class (--label2)")
    p.add_argument("--label2", default="")
    p.add_argument("--change", default="")
    p.add_argument("--file_root", default="", help="data set root in the reference's layout, instead of --pre / --post")
    p.add_argument("--split", default="test")
    p.add_argument("--out_dir", default="./scene_out")
    p.add_argument("--stride", type=int, default=None, help="tile stride; default: half the tile")
    p.add_argument("--window", choices=["hann", "flat"], default="hann")
    p.add_argument("--batch_size", type=int, default=32, help="model inputs per forward (tiles times --tta views)")
    p.add_argument("--tta", choices=["none", "hflip", "flips", "d4"], default="none", help="test-time augmentation: average every "
                   "tile over these views (hflip: 2, flips: 4, d4: all 8 flips and rotations) on the device")
    p.add_argument("--act_dtype", choices=["f32", "bf16"], default="bf16")
    p.add_argument("--in_height", type=int, default=256)
    p.add_argument("--in_width", type=int, default=256)
    p.add_argument("--num_class", type=int, default=None, help="SCD classes (default 7) or BDA damage classes (default 5)")
    p.add_argument("--objects", action="store_true", help="also the connected objects of the mask (SCD: of the change mask), as objects/<name>.csv")
    p.add_argument("--min_area", type=int, default=1, help="--objects: drop objects with fewer pixels")
    p.add_argument("--connectivity", type=int, choices=[4, 8], default=8)
    p.add_argument("--polygons", action="store_true", help="--objects: also their outlines, as objects/<name>.geojson")
    p.add_argument("--max_rings", type=int, default=None, help="--polygons: rows of the ring table (default: 4 per object row)")
    p.add_argument("--max_vertices", type=int, default=None, help="--polygons: rows of the vertex list (default: 16 per ring row)")
    p.add_argument("--simplify", type=simplify_tolerance, default=None, metavar="TOL", help="--polygons: simplify the rings on the "
                   "device (Douglas-Peucker) with this tolerance in pixels, in [0, 1024]")
    p.add_argument("--simplify_shared", action="store_true", help="--simplify: cut the rings where three or more regions meet and simplify "
                   "every wall once for both neighbours; features get `neighbours` and `collapsed`, a collapsed outline is written "
                   "with a null geometry, and the run ends with a `shared:` line.  Not with --simplify_min_iou, --simplify_valid or "
                   "--simplify_clean")
    p.add_argument("--simplify_safe", action="store_true", help="--simplify_shared in rounds (c3d_outlines_simplify_safe): the arcs of "
                   "every crossing, overlap, vertex inside another edge and collapsed ring get a smaller tolerance of their own until a "
                   "round finds nothing.  Implies --simplify_shared; every feature gets `refined`, and the run ends with a `safe:` line")
    p.add_argument("--safe_rounds", type=int, default=None, help="--simplify_safe: the most rounds, in [1, 64] (default 8); a scene "
                   "that needs more ends the run with an error")
    p.add_argument("--simplify_check", action="store_true", help="--simplify: fill the simplified polygons back into pixels on the device "
                   "and join them to the raw objects: an `iou` per feature and a closing `simplify:` line")
    p.add_argument("--simplify_min_iou", type=unit_interval, default=None, metavar="F", help="--simplify: implies --simplify_check; an "
                   "object whose IoU with its simplified polygon is not above F, in [0, 1], keeps its raw vertices")
    p.add_argument("--shapes", action="store_true", help="--polygons: also the convex hull and the minimum-area rectangle of every "
                   "object, on the device (c3d_rings_hull): shape properties on every feature, objects/<name>.hulls.geojson and "
                   "objects/<name>.rects.geojson, and a closing `shapes:` line")
    p.add_argument("--regularize", action="store_true", help="--polygons --simplify TOL: also square every simplified ring to the axes "
                   "of its object's minimum-area rectangle, on the device (c3d_rings_regularize): objects/<name>.regular.geojson with "
                   "coordinates at 1/16 px and `regular` per feature, and a closing `regularize:` line")
    p.add_argument("--regularize_min_iou", type=unit_interval, default=None, metavar="F", help="--regularize: fill the regularised "
                   "polygons back into pixels on the device; an object whose IoU with them is not above F, in [0, 1], keeps its "
                   "simplified rings in objects/<name>.regular.geojson; every feature there gets `iou`")
    p.add_argument("--validity", action="store_true", help="--polygons: also test every polygon against itself on the device "
                   "(c3d_rings_valid): `valid`, `crossings`, `overlaps` and `touches` on every feature, of the coordinates that are "
                   "written, and a closing `validity[stage]:` line for the raw, the simplified and the regularised rings")
    p.add_argument("--simplify_valid", action="store_true", help="--simplify: implies --validity; an object whose simplified polygon "
                   "crosses or overlaps itself, or could not be checked, keeps its raw vertices")
    p.add_argument("--regularize_valid", action="store_true", help="--regularize: implies --validity; an object whose regularised "
                   "polygon crosses or overlaps itself, or could not be checked, keeps its simplified rings")
    p.add_argument("--conflicts", action="store_true", help="--polygons: also compare the polygons of different objects on the device "
                   "(c3d_rings_conflicts): `conflicts`, `conflict_with` and `shared_walls` on every feature, of the coordinates that "
                   "are written, and a closing `conflicts[stage]:` line for the raw, the simplified and the regularised rings")
    p.add_argument("--simplify_clean", action="store_true", help="--simplify: implies --conflicts; an object whose polygon crosses "
                   "another object's, or overlaps it in the same direction, keeps its raw vertices; the written table is checked "
                   "again until it is clean")
    p.add_argument("--regularize_clean", action="store_true", help="--regularize: implies --conflicts; such an object keeps in "
                   "objects/<name>.regular.geojson what the main file writes for it")
    p.add_argument("--clean_rounds", type=int, default=8, metavar="N", help="--simplify_clean, --regularize_clean: at most N rounds of "
                   "fall back and check again; objects still in conflict then end the run with an error")
    p.add_argument("--label_polygons", default="", metavar="FILE", help="BCD, BDA: the ground truth as polygons, a GeoJSON FeatureCollection "
                   "in pixel coordinates or an xBD label JSON, instead of label rasters; with --file_root a directory of <name>.json / "
                   "<name>.geojson.  Filled on the device (c3d_rings_fill); one ground-truth object per feature")
    p.add_argument("--polygon_scores", action="store_true", help="--label_polygons --objects --polygons: also score every matched polygon "
                   "against its labelled one on the device (c3d_rings_polis): PoLiS and the vertex-to-boundary Hausdorff distance of "
                   "the raw, the simplified and the regularised rings, objects/<name>.polis.csv and a closing `polygons[stage]:` line each")
    p.add_argument("--iou_thr", type=iou_threshold, default=0.5, help="--objects with labels: a predicted and a labelled object match iff "
                   "their IoU is strictly above this; in [0.5, 1)")
    p.add_argument("--boundary", type=boundary_radius, default=None, metavar="D", help="with labels: also the boundary scores, Boundary IoU "
                   "over bands of this width in pixels and the contour precision / recall / F1; in [1, 1024]")
    p.add_argument("--boundary_tol", type=boundary_radius, default=None, metavar="T", help="--boundary: the contour tolerance in pixels "
                   "(default: D)")
    p.add_argument("--split_objects", type=boundary_radius, default=None, metavar="R", help="--objects: split touching objects "
                   "(c3d_scene_split): erode the mask by R pixels, in [1, 1024], and grow what is left back inside the mask, so that "
                   "objects joined by a neck narrower than about 2 R come apart.  Only the prediction is split: the labels that "
                   "--objects scores against stay whole components")
    p.add_argument("--regions", choices=["pre", "post", "transition"], default=None, help="--task SCD --objects: label the regions "
                   "of equal class of the pre or the post class map, or of their from-to transitions (c3d_scene_regions), instead of the "
                   "components of the change mask: cls is the key, from / to the classes, regions/<name>.png the map")
    p.add_argument("--sieve", type=sieve_area, default=None, metavar="N", help="--regions: absorb every region below N pixels into "
                   "the neighbour it shares the longest border with, on the device (c3d_regions_sieve); --min_area drops instead")
    p.add_argument("--sieve_rounds", type=sieve_rounds, default=None, metavar="R", help="--sieve: the most rounds, default 8")
    p.add_argument("--split_rounds", type=split_rounds, default=None, metavar="N", help="--split_objects: the most growth rounds, "
                   "in [1, 65536] (default 32); a scene that needs more ends the run with an error")
    p.add_argument("--pretrained", default="./pretrained/X3D_L.pyth")
    p.add_argument("--gpu_id", default=0, type=int)
    return p


if __name__ == "__main__":
    main()
