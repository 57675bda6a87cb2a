"""Vector ground truth: polygon files read into the ring table that `ops.rings_fill` (`c3d_rings_fill`) takes.  Host only, no
dependency beyond numpy and `json`.

`read_polygons(path, frac_bits=4)` reads

* a GeoJSON `FeatureCollection` of `Polygon` / `MultiPolygon` geometries in pixel coordinates -- what `predict_scene
  --polygons` writes; `properties.cls` is optional and defaults to 1 --, or
* an xBD label JSON: `features.xy[*].wkt` holding `POLYGON ((x y, ...), (hole), ...)`, read with the small parser below, the
  class from `properties.subtype`: no-damage 1, minor-damage 2, major-damage 3, destroyed 4, un-classified 1 (a pre-disaster
  file names no subtype: every building is 1).

Ids follow feature order, 1, 2, ...; holes, and the further polygons of a `MultiPolygon`, are further rings of the same id
(even-odd makes a hole of a ring inside another).  Coordinates are rounded to the nearest 2^-frac_bits pixel, ties to even.
The repeat of the first vertex that closes a ring in both formats is dropped.

The fill's rule is centre sampling: a pixel belongs to a polygon iff its centre lies inside (include/change3d_hip.h).  That
is NOT `cv2.fillPoly`'s rule, which also paints every pixel the boundary passes through, so a raster made with it is up to a
pixel fatter along every edge."""
import json
import re

import numpy as np

XBD_SUBTYPES = {"no-damage": 1, "minor-damage": 2, "major-damage": 3, "destroyed": 4, "un-classified": 1}
COORD_UNITS = 32768                                       # |coordinate| <= COORD_UNITS pixels, the limit of c3d_rings_fill

_NUMBER = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
_WKT_POLYGON = re.compile(r"^\s*POLYGON\s*(?:Z\s*|M\s*|ZM\s*)?\(\s*(.*)\)\s*$", re.IGNORECASE | re.DOTALL)
_WKT_RING = re.compile(r"\(([^()]*)\)")


class PolygonFileError(ValueError):
    pass


def parse_wkt_polygon(text):
    """The rings of `POLYGON ((x y, x y, ...), (...))` as lists of (x, y) floats; further ordinates of a point are ignored."""
    m = _WKT_POLYGON.match(text)
    if not m:
        raise PolygonFileError(f"not a WKT POLYGON: {text[:60]!r}")
    body = m.group(1)
    if re.sub(r"[\s,]", "", _WKT_RING.sub("", body)):
        raise PolygonFileError(f"unexpected text between the rings of {text[:60]!r}")
    rings = []
    for ring in _WKT_RING.findall(body):
        points = []
        for point in ring.split(","):
            parts = point.split()
            if len(parts) < 2 or not all(re.fullmatch(_NUMBER, p) for p in parts):
                raise PolygonFileError(f"bad point {point.strip()!r} in {text[:60]!r}")
            points.append((float(parts[0]), float(parts[1])))
        rings.append(points)
    if not rings:
        raise PolygonFileError(f"a POLYGON without rings: {text[:60]!r}")
    return rings


def _geojson_rings(geometry):
    kind = geometry.get("type") if isinstance(geometry, dict) else None
    coords = geometry.get("coordinates") if isinstance(geometry, dict) else None
    if kind == "Polygon":
        polygons = [coords]
    elif kind == "MultiPolygon":
        polygons = coords
    else:
        raise PolygonFileError(f"geometry type {kind!r}: only Polygon and MultiPolygon are read")
    rings = []
    for polygon in polygons:
        for ring in polygon:
            points = []
            for point in ring:
                if not isinstance(point, (list, tuple)) or len(point) < 2 or not all(isinstance(c, (int, float)) for c in point[:2]):
                    raise PolygonFileError(f"bad position {point!r}")
                points.append((float(point[0]), float(point[1])))
            rings.append(points)
    return rings


def _features(doc):
    """[(rings, cls)] in feature order, from either format."""
    if not isinstance(doc, dict) or "features" not in doc:
        raise PolygonFileError("neither a GeoJSON FeatureCollection nor an xBD label file: no `features`")
    feats = doc["features"]
    xbd = isinstance(feats, dict)
    if xbd:
        if "xy" not in feats:
            raise PolygonFileError("an xBD label file without `features.xy`")
        feats = feats["xy"]
    out = []
    for k, feat in enumerate(feats):
        try:
            props = (feat.get("properties") or {}) if isinstance(feat, dict) else None
            if props is None:
                raise PolygonFileError("not an object")
            if xbd:
                rings = parse_wkt_polygon(feat["wkt"]) if isinstance(feat.get("wkt"), str) else None
                if rings is None:
                    raise PolygonFileError("no `wkt` string")
                subtype = props.get("subtype", "no-damage")
                if subtype not in XBD_SUBTYPES:
                    raise PolygonFileError(f"unknown subtype {subtype!r}")
                cls = XBD_SUBTYPES[subtype]
            else:
                rings = _geojson_rings(feat.get("geometry"))
                cls = props.get("cls", 1)
                if isinstance(cls, bool) or not isinstance(cls, int) or not 0 <= cls <= 255:
                    raise PolygonFileError(f"properties.cls = {cls!r} is no class in [0, 255]")
        except PolygonFileError as e:
            raise PolygonFileError(f"feature {k}: {e}") from None
        out.append((rings, cls))
    return out


def polygons_table(features, frac_bits=4):
    """`(rings i32 [R, 8], vertices i32 [V, 2], counts i32 [5], id_cls u8 [N])` from [(rings of (x, y) floats, cls)]: feature k
    gets id k + 1.  R and V are at least 1, so that the arrays can go to the device as they are."""
    if not 0 <= int(frac_bits) <= 8:
        raise ValueError(f"frac_bits must lie in [0, 8], got {frac_bits}")
    scale, limit = float(1 << frac_bits), COORD_UNITS << frac_bits
    rows, verts, classes = [], [], []
    for k, (rings, cls) in enumerate(features):
        classes.append(cls)
        for ring in rings:
            q = np.rint(np.asarray(ring, dtype=np.float64).reshape(-1, 2) * scale)
            if not np.isfinite(q).all() or (np.abs(q) > limit).any():
                raise PolygonFileError(f"feature {k}: a coordinate lies outside [-{COORD_UNITS}, {COORD_UNITS}] pixels")
            q = q.astype(np.int64)
            if len(q) > 1 and (q[0] == q[-1]).all():
                q = q[:-1]
            rows.append((k + 1, sum(len(v) for v in verts), len(q), 0, 0, 0, 0, 0))
            verts.append(q)
    total = sum(len(v) for v in verts)
    rings_a = np.zeros((max(len(rows), 1), 8), dtype=np.int32)
    if rows:
        rings_a[:len(rows)] = np.asarray(rows, dtype=np.int64)
    vertices = np.zeros((max(total, 1), 2), dtype=np.int32)
    if total:
        vertices[:total] = np.concatenate(verts)
    counts = np.array([len(rows), len(rows), total, total, 0], dtype=np.int32)
    return rings_a, vertices, counts, np.asarray(classes, dtype=np.uint8).reshape(-1)


def read_polygons(path, frac_bits=4):
    """The polygons of a GeoJSON or xBD label file as `(rings, vertices, counts, id_cls)` numpy arrays for `ops.rings_fill`
    (see the module's text).  Raises `PolygonFileError` naming the feature's index on anything it cannot read and on a
    coordinate out of range."""
    with open(path) as f:
        try:
            doc = json.load(f)
        except json.JSONDecodeError as e:
            raise PolygonFileError(f"{path}: not JSON ({e})") from None
    try:
        return polygons_table(_features(doc), frac_bits)
    except PolygonFileError as e:
        raise PolygonFileError(f"{path}: {e}") from None
