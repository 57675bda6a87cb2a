"""c3d_rings_fill on the MI355X at 1024 x 1024, 8-connectivity, on the masks of tools/outlines_step.py (blobs, random at density
0.59, all foreground, serpentine, checkerboard): the raw rings of c3d_scene_outlines and the rings simplified at 1 px filled back
into a label map, timed with device events around repeated calls after a warm-up, median over several rounds, in one process,
next to the c3d_scene_outlines call on the same mask.  The raw fill must give the labels back; the script says so.  Then the
host way, once each: the download of the ring table and the vertices, the numpy restatement of the rule
(tests/fill_reference.py; only where the rings have at most HOST_EDGES edges -- it is a brute force and takes a second per ten
thousand edges), and PIL.ImageDraw.polygon, outlines in id order and then holes painted 0, with the share of pixels on which it
agrees (PIL also paints the pixels under the boundary, and a hole painted 0 erases an object that lies inside it).  Writes
stdout (`python tools/fill_step.py > profiles/rings_fill.txt`)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402

HOST_EDGES = 40000


def host_way(rings, vertices, counts, labels_np, max_objects):
    import fill_reference
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r, v, c = rings.cpu().numpy(), vertices.cpu().numpy(), counts.cpu().numpy()
    t_down = (time.perf_counter() - t0) * 1e6
    rows, edges = int(c[1]), int(c[3])
    line = f"              host: download of the tables {t_down:10.1f} us;  "
    if edges <= HOST_EDGES:
        t0 = time.perf_counter()
        want = fill_reference.fill(r, v, c, S, S, 0, None, max_objects)["labels"]
        line += f"numpy restatement {(time.perf_counter() - t0) * 1e6:12.1f} us ({'equal' if np.array_equal(want, labels_np) else 'DIFFERENT'});  "
    else:
        line += f"numpy restatement not run ({edges} edges);  "
    try:
        from PIL import Image, ImageDraw
        t0 = time.perf_counter()
        img = Image.new("I", (S, S), 0)
        draw = ImageDraw.Draw(img)
        order = sorted(range(rows), key=lambda k: (r[k, 3] <= 0, r[k, 0]))   # the outlines in id order, then the holes
        for k in order:
            if r[k, 1] >= 0 and r[k, 2] >= 3:
                draw.polygon([tuple(p) for p in v[r[k, 1]:r[k, 1] + r[k, 2]].tolist()], fill=int(r[k, 0]) if r[k, 3] > 0 else 0)
        got = np.asarray(img, dtype=np.int32)
        line += f"PIL.ImageDraw.polygon {(time.perf_counter() - t0) * 1e6:12.1f} us, agrees on {(got == labels_np).mean() * 100:.2f} % of the pixels"
    except ImportError:
        line += "PIL not installed"
    print(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/fill_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    nbytes = L.lib().c3d_rings_fill_ws_bytes(max_rings, max_vertices, max_objects, S, S)
    print(f"# tools/fill_step.py: {S} x {S}, 8-connectivity, frac_bits 0; workspace {nbytes / 2**20:.1f} MiB; tier limits "
          f"{ops.rings_fill_limits()}; device events, {ROUNDS} rounds of 20 calls, median (min .. max); {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_o = torch.empty(L.lib().c3d_scene_outlines_ws_bytes(S, S), dtype=torch.uint8, device=dev)
    yy, xx = np.mgrid[0:S, 0:S]
    for name, mask_np in masks() + [("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8))]:
        mask = torch.from_numpy(mask_np).to(dev)
        labels, table, _, _, counts_obj = ops.scene_objects(mask, connectivity=8, max_objects=max_objects, want_object_cls=False)
        trace = lambda: ops.scene_outlines(labels, counts_obj, connectivity=8, max_objects=max_objects, max_rings=max_rings,  # noqa: E731
                                           max_vertices=max_vertices, ws=ws_o)
        raw = trace()
        simple = ops.outlines_simplify(*raw, 1.0)
        fill_raw = lambda: ops.rings_fill(*raw, S, S, max_objects=max_objects, ws=ws)  # noqa: E731
        fill_simple = lambda: ops.rings_fill(*simple, S, S, max_objects=max_objects, ws=ws)  # noqa: E731
        back, table_b, _, _, _, info = fill_raw()
        s_labels, s_table, _, _, _, s_info = fill_simple()
        torch.cuda.synchronize()
        objects = int(counts_obj[0])
        box = table[:objects, 3:5] - table[:objects, 1:3] + 1
        large = int(((box[:, 0] > ops.rings_fill_limits()[0]) | (box[:, 1] > ops.rings_fill_limits()[0])).sum()) if objects else 0
        ok = torch.equal(back, labels) and torch.equal(table_b[:, :5], table[:, :5])
        print(f"{name:12s}: density {mask_np.mean():.2f}, {objects} objects ({large} in the workgroup tier), {int(raw[2][0])} rings, "
              f"{int(raw[2][2])} vertices raw, {int(simple[2][2])} at 1 px; status {int(info[0])} / {int(s_info[0])}; the raw fill gives the "
              f"labels back: {'yes' if ok else 'NO'}; at 1 px {int((s_labels != labels).sum())} pixels differ, "
              f"{int((s_table[:objects, 0] == 0).sum()) if objects else 0} objects vanish")
        t_raw, t_simple, t_trace = event_us(fill_raw), event_us(fill_simple), event_us(trace)
        print(f"              fill raw {t_raw[0]:8.1f} us ({t_raw[1]:.1f} .. {t_raw[2]:.1f})  {S * S / t_raw[0]:7.1f} Mpx/s;  fill at 1 px "
              f"{t_simple[0]:8.1f} us ({t_simple[1]:.1f} .. {t_simple[2]:.1f});  c3d_scene_outlines {t_trace[0]:8.1f} us "
              f"({t_trace[1]:.1f} .. {t_trace[2]:.1f}): the raw fill costs {t_raw[0] / t_trace[0]:.2f} of it")
        host_way(*raw, labels.cpu().numpy(), max_objects)


if __name__ == "__main__":
    main()
