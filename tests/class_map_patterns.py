"""Hand-drawn maps for the class-activation region tests (tests/test_class_maps_cpu.py on the host restatement, tests/test_gpu_class_maps.py on the
kernel) and an independent breadth-first search that says what their peak, box and area are.  Nothing here calls the library."""
from collections import deque

import numpy as np

FRACS = (0.0, 0.2, 0.5, 1.0)


def _serpentine(n=9, path=5, peak=9):
    """a one-cell-wide path through an n x n grid: the even rows in full, joined at alternating ends; the peak at its start.  Growing it from
    the peak takes a sweep per cell of the path when a sweep only sees the previous sweep's cells"""
    m = np.zeros((n, n), dtype=np.float32)
    m[0::2, :] = path
    for r in range(1, n, 2):
        m[r, n - 1 if (r // 2) % 2 == 0 else 0] = path
    m[0, 0] = peak
    return m


def _two_blobs():
    m = np.full((6, 8), -3, dtype=np.float32)
    m[0:2, 0:2] = [[5, 6], [7, 6]]                     # the lower blob in value ...
    m[3:5, 4:7] = [[8, 9, 8], [8, 8, 7]]               # ... and the peak's blob, which wins
    return m


def _diagonal():
    return np.array([[9, 9, 0, 0], [9, 8, 0, 0], [0, 0, 8, 8], [0, 0, 8, 8]], dtype=np.float32)     # (1, 1) and (2, 2) touch by a corner only


def _plateau():
    m = np.ones((5, 5), dtype=np.float32)
    m[3, 2] = m[1, 3] = m[1, 1] = 7                    # tied maxima: (1, 1) has the lowest y W + x
    m[1, 2] = 4                                        # joins (1, 1) and (1, 3) at frac <= 0.5
    return m


def _borders():
    m = np.zeros((6, 7), dtype=np.float32)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 6        # a ring on all four borders
    m[5, 6] = 8
    return m


def _frac1_above_max():
    """mn = -2^-25, mx = 1 - 2^-24: mx - mn = 1 - 2^-25 is a tie that rounds to even, 1.0; mn + 1.0 is the same tie: tau = 1.0 > mx"""
    mx, mn = np.float32(1.0) - np.float32(2.0 ** -24), -np.float32(2.0 ** -25)
    m = np.full((3, 4), mn, dtype=np.float32)
    m[1, 2] = mx
    m[1, 1] = m[0, 2] = mx                             # other cells AT the maximum: below tau, so not in the region
    return m


# name -> (map float32 [H, W], every value a small integer?)
PATTERNS = {
    "two_blobs": (_two_blobs(), True),
    "diagonal": (_diagonal(), True),
    "serpentine9": (_serpentine(), True),
    "plateau": (_plateau(), True),
    "constant": (np.full((4, 5), 3, dtype=np.float32), True),
    "borders": (_borders(), True),
    "one_cell": (np.array([[4]], dtype=np.float32), True),
    "row7": (np.array([[1, 5, 5, 0, 9, 9, 2]], dtype=np.float32), True),
    "frac1_above_max": (_frac1_above_max(), False),
}


def tau_of(mn, mx, frac):
    """mn + frac (mx - mn), each operation rounded to float32"""
    f = np.float32
    return f(f(mn) + f(f(frac) * f(f(mx) - f(mn))))


def bfs_region(m, frac):
    """-> ((peak_y, peak_x, y0, x0, y1, x1, area, 0), (mn, mx)) of one map by a queue-based search with python loops"""
    m = np.asarray(m, dtype=np.float32)
    h, w = m.shape
    best, py, px, mn = None, 0, 0, None
    for y in range(h):
        for x in range(w):
            v = m[y, x]
            if best is None or v > best:
                best, py, px = v, y, x
            if mn is None or v < mn:
                mn = v
    tau = tau_of(mn, best, frac)
    seen = {(py, px)}
    todo = deque(seen)
    while todo:
        y, x = todo.popleft()
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < h and 0 <= nx < w and (ny, nx) not in seen and m[ny, nx] >= tau:
                seen.add((ny, nx))
                todo.append((ny, nx))
    ys, xs = [p[0] for p in seen], [p[1] for p in seen]
    return (py, px, min(ys), min(xs), max(ys), max(xs), len(seen), 0), (mn, best)
