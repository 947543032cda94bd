"""What the cursor kernels compute, stepped on the oracle one symbol at a time: the depth profile of fmgpu_search_exact_depth and the single-symbol steps of
fmgpu_cursor_extend.  Shared by tests/test_gpu_cursor_steps.py and tests/test_gpu_superblocks.py."""
import numpy as np

import fmoracle as fo


def depth_model(ox, reads):
    """include/fmgpu.h on fmgpu_search_exact_depth, sentence by sentence: step the cursor leftwards from the read's last symbol while it holds more than one row and
    count the symbols consumed; a symbol >= sigma counts and empties the cursor; length + 1 if several rows remain at the end"""
    sigma = ox.sigma
    out = np.zeros(len(reads), dtype=np.uint64)
    for q, read in enumerate(reads):
        cur = ox.cursor()
        rows, consumed = int(cur.len), 0
        for c in read[::-1]:
            if rows <= 1:
                break
            consumed += 1
            if int(c) >= sigma:
                rows = 0
                break
            cur = ox.extend_left(cur, int(c))
            rows = int(cur.len)
        out[q] = consumed if rows <= 1 else len(read) + 1
    return out


def single_steps(ox, cursors, right):
    """extendLeft(c) / extendRight(c) of every cursor {lb, lb_rev, len} for every symbol c, one oracle call each: (cursors, sigma, 3)"""
    step = ox.extend_right if right else ox.extend_left
    out = np.zeros((len(cursors), ox.sigma, 3), dtype=np.uint64)
    for k, (a, r, l) in enumerate(cursors):
        for c in range(ox.sigma):
            nc = step(fo.Cursor(int(a), int(r), int(l)), c)
            out[k, c] = (nc.lb, nc.lb_rev, nc.len)
    return out
