"""The run partition of a persistent LVC launch (fd_lvc_ps_partition, FD_OPT_LVC_CARRY): host only."""
import ctypes as C
import random

from prodiff_amd import _lib


def partition(rows, batch, grid):
    n = C.c_int()
    _lib.check(_lib.lib().fd_lvc_ps_partition(rows, batch, grid, None, 0, C.byref(n)))
    buf = (C.c_int * (3 * max(n.value, 1)))()
    _lib.check(_lib.lib().fd_lvc_ps_partition(rows, batch, grid, buf, n.value, C.byref(n)))
    return [tuple(buf[3 * i:3 * i + 3]) for i in range(n.value)]


def tile_times(t0, t1):
    """Tiles a block spends on the run [t0, t1): its first tile yields 384 rows (448 at row 0), later ones 448."""
    first = 448 if t0 == 0 else 384
    return 1 + max(0, -(-(t1 - t0 - first) // 448))


def makespan(runs, grid):
    """Block v walks runs v, v + grid, ... (the kernel's XCD-aware order permutes the runs among the blocks,
    not their lengths; with one run per block the makespan is the longest run)."""
    return max(sum(tile_times(t0, t1) for _, t0, t1 in runs[v::grid]) for v in range(grid))


def test_partition_tiles_every_row_once():
    rng = random.Random(5)
    shapes = [(768, 1, 1), (5888, 3, 4), (2560, 2, 5), (2560, 2, 3), (64, 1, 1), (384, 4, 2), (448, 3, 1)]
    shapes += [(64 * rng.randint(1, 4000), rng.randint(1, 9), rng.randint(1, 300)) for _ in range(300)]
    for rows, batch, grid in shapes:
        runs = partition(rows, batch, grid)
        ntiles = -(-rows // 384) * batch
        if ntiles <= grid:
            assert runs == [], (rows, batch, grid)      # one tile per block: nothing to carry
            continue
        assert len(runs) == max(grid, batch)
        per = {}
        for b, t0, t1 in runs:
            assert 0 <= b < batch and 0 <= t0 < t1 <= rows, (rows, batch, grid, b, t0, t1)   # inside one utterance
            assert t0 % 64 == 0 and (t1 % 64 == 0 or t1 == rows)
            per.setdefault(b, []).append((t0, t1))
        assert sorted(per) == list(range(batch))
        for b, rs in per.items():                        # consecutive, in time order, covering [0, rows) once
            assert rs[0][0] == 0 and rs[-1][1] == rows
            assert all(x[1] == y[0] for x, y in zip(rs, rs[1:]))
        assert [b for b, _, _ in runs] == sorted(b for b, _, _ in runs)


def test_partition_c3_makespan():
    """C3 on 256 CUs: 8 x 220 416 rows in 16 tile-times (18 with 384-row tiles), 8 x 55 104 in 4 (5)."""
    assert makespan(partition(861 * 256, 8, 256), 256) == 16
    assert makespan(partition(861 * 64, 8, 256), 256) == 4
