"""Edge matrices for the PACKED form of the row-chunk kernel (csrc/dsgd_fstep.hpp, dsgd_fstep_kernel<true>): small CSR matrices
built by CONSTRUCTION, not drawn, so that the windows a wave rebuilds in registers (w_tile_q<..., true>, csrc/dsgd_kernels.hpp)
meet every edge of their arithmetic.  Plain numpy: tests/test_packed_edges.py cuts them on the CPU with the project's own
builders (tests/cpp/packed_edges_test.cpp: the witness that says which tile shapes each matrix produces),
tests/test_gpu_packed_edges.py runs them on the device.

A fixed set of HOT_N columns is hot by use -- every hot key occurs in hundreds of rows, no cold key in more than a few dozen --
and DSGD_HSPLIT = HOT_N makes that set the hot stream: a row's length THERE is what the pattern below chooses.

  phases   8,192 rows = 128 blocks of 64 rows.  Every block holds 641 hot slots (641 = 1 mod 8: block b starts at slot phase
           b mod 8, all eight phases in turn) and the same number of cold slots, so every block weighs the same when the rows are
           cut into chunks: with DSGD_FSTEP_ROWS=64 and one worker the 128 chunks ARE the blocks (=512: eight blocks each).
           A block is  hot lengths 1..7 (rotated by v = (b div 8) mod 8)  |  45 - v longer rows that end exactly 511 slots
           behind the block's window start (the largest tile the builders cut)  |  12 rows  |  v rows of one slot  -- the last
           v starts lie in front of the next block's first row.  Every second v puts a row of 80 slots (more than eight lanes)
           among the longer ones.  hot_nnz = 128 * 641 is a multiple of 8.
  ragged   ~4,100 rows, not block-aligned on purpose: tiled rows of two slots between two rows of the long list at every
           phase (tiles of fewer than 8 slots), empty rows and rows with cold entries only between rows with hot entries, 900
           rows of one slot (the 254-row cap) and 600 of two or three (more than 64 rows per tile), four long rows in a row
           (chunks without a hot tile; RAGGED_LONG_RUN names the first: a range that STARTS there has no tile in its first
           chunk), ordinary rows of 5..40 slots.  hot_nnz is no multiple of 8.

Labels: "mixed" (a fixed pattern of both), "neg" (all -1), "pos" (all +1), "alt" (alternating)."""

from __future__ import annotations

import numpy as np

from dsgd_amd import synth

DIM = 4000
HOT_N = 128                                                   # = DSGD_HSPLIT (a multiple of 4: dsgd_create keeps it)
HOT_KEYS = (3 + 29 * np.arange(HOT_N)).astype(np.int32)       # 3, 32, ..., 3686: spread over the keys
COLD_KEYS = np.setdiff1d(np.arange(1, DIM + 1, dtype=np.int32), HOT_KEYS)
LONG = (3, 600)                                               # a row of the long list: more than 504 cold entries
FSTEP_ROWS = ("64", "512")                                    # the DSGD_FSTEP_ROWS values of the witness and of the GPU tests
N_CU = 256                                                    # the MI355X's compute units (fstep_grid: workgroups per worker)
LABELS = ("mixed", "neg", "pos", "alt")


def _spread(total, n):
    """n lengths that sum to total, as equal as they can be"""
    base, rem = divmod(total, n)
    assert base >= 1
    return [base + 1] * rem + [base] * (n - rem)


def phases_rows():
    rows = []
    for b in range(128):
        s, v = b % 8, (b // 8) % 8
        head = list(np.roll(np.arange(1, 8), v))
        n1 = 45 - v
        first = ([80] + _spread(403 - s, n1 - 1)) if v % 2 == 0 else _spread(483 - s, n1)
        if v % 2 == 0:   # (the row of 80 slots in the middle of the longer ones)
            first = first[1:n1 // 2] + [80] + first[n1 // 2:]
        rest = _spread(130 - v + s, 12)
        block = head + first + rest + [1] * v
        assert len(block) == 64 and sum(block) == 641
        rows += [(int(h), i % 3) for i, h in enumerate(block)]
    return rows


def ragged_rows():
    rows = []
    for rep in range(24):
        rows += [(9 + rep % 8, 1)] * 3 + [(1, 1)] * (rep % 8) + [LONG, (2, 1), LONG, (6, 2), (0, 3), (7, 0), (0, 0), (4, 1),
                                                                  (0, 0), (0, 2), (11 + rep % 5, 1)]
    for i in range(900):
        rows.append([(1, 1), (0, 2), (1, 0), (1, 2)][i % 4] if i % 113 else (0, 0))
    for i in range(600):
        rows.append((2 + i % 2, i % 3))
    long_run = len(rows)
    rows += [LONG] * 4
    for i in range(2500):
        rows.append((5 + (i * 7) % 36, i % 4))
    hot = sum(max(h, 1) for h, c in rows if (h, c) != LONG)
    if hot % 8 == 0:
        rows.append((3, 1))
    return rows, long_run


RAGGED_LONG_RUN = ragged_rows()[1]


def labels_of(n_rows, mode):
    i = np.arange(n_rows)
    if mode == "neg":
        return np.full(n_rows, -1, np.int8)
    if mode == "pos":
        return np.full(n_rows, 1, np.int8)
    if mode == "alt":
        return np.where(i % 2 == 0, 1, -1).astype(np.int8)
    assert mode == "mixed"
    return np.where((i * 7 + i // 3) % 3 == 0, -1, 1).astype(np.int8)


def csr_of(rows, label_mode="mixed"):
    """rows: (hot entries, cold entries) per row.  Keys round-robin over the two sets (every hot key in about as many rows as
    any other), values of both signs in [1/16, 1] from a fixed multiplicative hash of the entry's position."""
    n_rows = len(rows)
    lens = np.array([h + c for h, c in rows], np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.empty(int(row_ptr[-1]), np.int32)
    hp = cp = 0
    for i, (h, c) in enumerate(rows):
        keys = np.concatenate([HOT_KEYS[(hp + np.arange(h)) % HOT_N], COLD_KEYS[(cp + np.arange(c)) % len(COLD_KEYS)]])
        hp += h
        cp += c
        col[row_ptr[i]:row_ptr[i + 1]] = np.sort(keys)
    e = np.arange(len(col), dtype=np.uint64)
    hsh = (e * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 32)
    mag = (16.0 + (hsh >> np.uint64(8)) % np.uint64(241)) / 256.0                    # 1/16 .. 1 + 1/256, on a grid of 2^-8
    val = np.where((hsh >> np.uint64(20)) % np.uint64(2) == 0, mag, -mag).astype(np.float32)
    return synth.Csr(DIM, row_ptr, col, val, labels_of(n_rows, label_mode))


_CACHE = {}


def matrix(name, label_mode="mixed"):
    key = (name, label_mode)
    if key not in _CACHE:
        rows = phases_rows() if name == "phases" else ragged_rows()[0]
        assert name in ("phases", "ragged") and len(rows) <= 8192
        _CACHE[key] = csr_of(rows, label_mode)
    return _CACHE[key]


def hot_mask(data):
    """[key] -> is the key one of the HOT_N most frequent?  Asserts the margin the witness relies on: every hot key occurs in
    far more rows than any cold one (ten times at least), so the device's frequency ranking cuts exactly here."""
    cnt = np.bincount(data.col, minlength=data.dim + 1)
    hot = np.zeros(data.dim + 1, bool)
    hot[HOT_KEYS] = True
    assert cnt[hot].min() >= 10 * max(1, cnt[~hot].max()), (cnt[hot].min(), cnt[~hot].max())
    return hot


def ranges_of(name):
    """the row ranges of a step, by name: one worker; three unequal ranges whose boundaries fall inside the swept blocks; for
    `ragged` also a range that starts on the run of long rows"""
    data = matrix(name)
    n = data.n_rows
    if name == "phases":
        return {"one": [(0, n)], "three": [(0, 2075), (2075, 5021), (5021, n)]}
    return {"one": [(0, n)], "three": [(0, 333), (333, 1900), (1900, n)], "from_long": [(RAGGED_LONG_RUN, n)]}


def n_wg_of(ranges, fstep_rows):
    """csrc/dsgd_route.hpp fstep_grid, for ranges above DSGD_FSTEP_MIN (the C++ witness calls the function itself)"""
    per_worker = max(1, N_CU // len(ranges))
    tot, smallest = sum(b - a for a, b in ranges), min(b - a for a, b in ranges)
    return max(1, min(per_worker, min(smallest, tot) // max(1, int(fstep_rows))))


def write_case(path, name, label_mode="mixed"):
    """the matrix and its configurations as the witness reads them: int64 n_rows, nnz, dp, hot_n, n_cfg; row_ptr (int64), col
    (int32), label (int8), hot mask by key (uint8); per configuration int64 fstep_rows, n_ranges, then the ranges"""
    data = matrix(name, label_mode)
    hot = hot_mask(data)
    cfgs = [(int(r), rg) for r in FSTEP_ROWS for rg in ranges_of(name).values()]
    with open(path, "wb") as f:
        np.array([data.n_rows, data.nnz, data.dim + 1, HOT_N, len(cfgs)], np.int64).tofile(f)
        data.row_ptr.astype(np.int64).tofile(f)
        data.col.astype(np.int32).tofile(f)
        data.label.astype(np.int8).tofile(f)
        hot.astype(np.uint8).tofile(f)
        for r, rg in cfgs:
            np.array([r, len(rg)] + [x for ab in rg for x in ab], np.int64).tofile(f)
    return cfgs
