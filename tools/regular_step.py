"""c3d_rings_regularize on the MI355X at 1024 x 1024, 8-connectivity, on the masks of tools/objects_step.py plus the checkerboard
(and the serpentine, where those masks do not hold it already): the rings of c3d_scene_outlines simplified at 1 px, the hulls of
the raw rings, then the regularisation at 1/16 px, timed with device events around repeated calls after a warm-up, median over
several rounds, in one process, next to the c3d_outlines_simplify call it follows on the same mask.  Per mask also the rings
regularised and copied, per tier.  Writes stdout (`python tools/regular_step.py > profiles/rings_regularize.txt`)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402

TOL = 1.0


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/regular_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    nbytes = L.lib().c3d_rings_regularize_ws_bytes(max_rings, max_vertices, max_objects)
    wave, lds = ops.rings_regularize_limits()
    print(f"# tools/regular_step.py: {S} x {S}, 8-connectivity, simplified at {TOL:g} px, frac_bits 4; workspace {nbytes / 2**20:.1f} MiB; "
          f"tier limits {(wave, lds)}; device events, {ROUNDS} rounds of 20 calls, median (min .. max); {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_s = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices), dtype=torch.uint8, device=dev)
    yy, xx = np.mgrid[0:S, 0:S]
    todo = masks() + [("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8))]
    if not any(name.strip() == "serpentine" for name, _ in todo):
        snake = np.zeros((S, S), np.uint8)
        snake[::2] = 1
        for k, y in enumerate(range(1, S, 2)):
            snake[y, S - 1 if k % 2 == 0 else 0] = 1
        todo.append(("serpentine", snake))
    for name, mask_np in todo:
        mask = torch.from_numpy(mask_np).to(dev)
        labels, table, _, _, counts_obj = ops.scene_objects(mask, connectivity=8, max_objects=max_objects, want_object_cls=False)
        raw = ops.scene_outlines(labels, counts_obj, connectivity=8, max_objects=max_objects, max_rings=max_rings, max_vertices=max_vertices)
        simplify = lambda: ops.outlines_simplify(*raw, TOL, ws=ws_s)  # noqa: E731
        simple = simplify()
        hull = ops.rings_hull(*raw, max_objects=max_objects)
        regular = lambda: ops.rings_regularize(*simple, *hull, frac_bits=4, ws=ws)  # noqa: E731
        rings, vertices, counts = regular()
        torch.cuda.synchronize()
        rows = rings[:int(counts[1])]
        used = rows[:, 1] >= 0
        flag, n_in, n_out = rows[:, 3] == 1, rows[:, 7], rows[:, 2]
        tier = lambda lo, hi: (int((used & flag & (n_in > lo) & (n_in <= hi)).sum()), int((used & ~flag & (n_in > lo) & (n_in <= hi)).sum()))  # noqa: E731
        t_wave, t_lds, t_hbm = tier(-1, wave), tier(wave, lds), tier(lds, 1 << 30)
        print(f"{name:12s}: density {mask_np.mean():.2f}, {int(hull[3][0])} objects, {int(counts[1])} rings, {int(raw[2][2])} raw vertices, "
              f"{int(simple[2][2])} simplified, {int(counts[2])} out (the longest simplified ring has {int(n_in.max()) if len(rows) else 0}, "
              f"the longest regularised {int(n_out[flag].max()) if bool(flag.any()) else 0}); status {int(counts[4])}")
        print(f"              regularised / copied: wave tier {t_wave[0]} / {t_wave[1]}, LDS tier {t_lds[0]} / {t_lds[1]}, "
              f"HBM tier {t_hbm[0]} / {t_hbm[1]}")
        t_reg, t_sim = event_us(regular), event_us(simplify)
        print(f"              regularize {t_reg[0]:8.1f} us ({t_reg[1]:.1f} .. {t_reg[2]:.1f});  c3d_outlines_simplify {t_sim[0]:8.1f} us "
              f"({t_sim[1]:.1f} .. {t_sim[2]:.1f}): the regularisation costs {t_reg[0] / t_sim[0]:.2f} of it")


if __name__ == "__main__":
    main()
