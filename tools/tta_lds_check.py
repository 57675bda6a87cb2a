"""Bank check of the LDS block of the test-time-augmentation kernels (csrc/scene_ops.hip, scene_gather_views_kernel and
scene_fold_views_kernel) with the cycle model of lds_bank_model.py.

The block is [32][pitch] dwords.  Lane l of a wave is (r, q) = (r0 + (l >> 3), l & 7): it writes the words k = 0 .. 3 of its
quad by rows, at r * pitch + 4q + k, and reads the transposed quad by columns, at (4q + k) * pitch + r, one dword per access
(the `r32` rule -- banks modulo 32 dwords, the two 32-lane halves -- holds for ds_write_b32 and ds_read_b32 alike).  Two
cycles per wave access is the conflict-free floor: one per half."""
from lds_bank_model import cycles


def block_cycles(pitch, r0=0):
    """(worst cycles of a row-order access, worst cycles of a column-order access) over the four words of a quad."""
    rows = max(cycles(lambda l, k=k: ((r0 + (l >> 3)) * pitch + 4 * (l & 7) + k) * 4, "r32") for k in range(4))
    cols = max(cycles(lambda l, k=k: ((4 * (l & 7) + k) * pitch + r0 + (l >> 3)) * 4, "r32") for k in range(4))
    return rows, cols


if __name__ == "__main__":
    for pitch in (32, 33, 36):
        worst = [block_cycles(pitch, r0) for r0 in range(0, 32, 8)]     # the four waves of a workgroup
        print(f"pitch {pitch}: by rows {max(w[0] for w in worst)} cycles, by columns {max(w[1] for w in worst)} cycles per wave access "
              f"(floor 2)")
