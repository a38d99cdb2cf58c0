"""No GPU needed: the CPU witness of the packed form's edge matrices (tests/packed_edge_data.py).

tests/cpp/packed_edges_test.cpp, compiled with AddressSanitizer and UBSan and run as a program of its own, reads each matrix as
this module writes it, cuts it with the project's builders (split_offsets, fstep_grid, cut_row_chunks, packed_streams_ref) at
the DSGD_FSTEP_ROWS values and row ranges that tests/test_gpu_packed_edges.py runs on the device, holds packed_lane_bits to the
lane descriptors on every tile and on the padding tiles of short chunks, and prints how many tiles fall into each edge class.
This module asserts that every class is met -- so a green run of the GPU tests on these matrices says that the kernel's
register arithmetic was right ON those shapes, not that no such shape came up -- and that every deliberately wrong reader in
the program differs from the descriptors somewhere.

Two things the issue behind these tests assumed do not hold, and the program says so instead of dropping them:

  * the largest tile has 511 slots, not 512 (append_wave_tiles closes a tile at WS_SLOTS - 1), so `n >> 3` always names a lane:
    the nearest shape is the end mark in lane 63, bit 7, and that is asserted;
  * masking the end-mark lane with `em - 1` instead of `em - 1 + em` is the SAME reader (the end mark is or-ed in right behind
    the mask): the program checks the identity for all 256 x 8 inputs and asserts that this variant never differs; the masks
    that are wrong -- one slot too wide, none at all -- are asserted to differ instead.

Rows without hot entries DO own a tile row (one explicit-zero slot), so that class is reached as asked."""

import os
import subprocess

import pytest

import packed_edge_data as pe
from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")

# class -> the matrices that must reach it (every class by at least one; most by both)
BOTH = ("phases", "ragged")
CLASSES = {
    "end_mark_on_8_below_cap": BOTH, "largest_tile_511": ("phases",),
    "extra_1": BOTH, "extra_2": BOTH, "extra_3": BOTH, "extra_4": BOTH, "extra_5": BOTH, "extra_6": BOTH, "extra_7": ("phases",),
    "tiny_tile_with_extra": ("ragged",), "rows_over_64": ("ragged",), "rows_at_cap_254": ("ragged",),
    "last_tile_stream_mult8": ("phases",), "last_tile_stream_not_mult8": ("ragged",),
    "chunk_under_16_tiles": BOTH, "chunk_without_tiles": ("ragged",), "first_chunk_without_tiles": ("ragged",),
    "row_start_in_slot_7": BOTH, "row_over_8_lanes": ("phases",), "general_path_tiles": BOTH, "flag_right_behind_end_mark": BOTH,
    "padding_tiles_checked": BOTH,
    "long_row_before_a_tiled_row": ("ragged",), "long_row_after_a_tiled_row": ("ragged",),
    "empty_row_between_hot_rows": ("ragged",), "cold_only_row_between_hot_rows": ("ragged",),
}
WRONG_READERS = ("no_extra_drop", "mask_one_slot_wide", "no_mask", "keep_255_on_padding")


@pytest.fixture(scope="module")
def witness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("packed_edges") / "packed_edges_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "packed_edges_test.cpp"), "-o", exe], check=True)
    return exe


def run_witness(exe, tmp_path, name, label_mode):
    path = str(tmp_path / ("%s_%s.bin" % (name, label_mode)))
    pe.write_case(path, name, label_mode)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print("---- %s, labels %s" % (name, label_mode))
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "all checks passed" in r.stdout
    total, mutant = {}, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "TOTAL":
            total[w[1]] = int(w[2])
        elif w and w[0] == "MUTANT":
            mutant[w[1]] = int(w[2])
    return total, mutant, r.stdout


def test_the_matrices_are_what_the_witness_assumes():
    for name in ("phases", "ragged"):
        data = pe.matrix(name)
        assert data.n_rows <= 8192 and data.dim == pe.DIM
        hot = pe.hot_mask(data)   # (asserts the margin between the hot and the cold keys' counts)
        assert hot.sum() == pe.HOT_N and pe.HOT_N % 4 == 0
        assert (hot[data.col] == 0).sum() > 0 and data.dim + 1 - pe.HOT_N < 65536   # a cold stream of 16-bit ids
        for i in range(0, data.n_rows, 97):   # ascending keys, no key twice
            k = data.col[data.row_ptr[i]:data.row_ptr[i + 1]]
            assert (k[1:] > k[:-1]).all()
        for mode in pe.LABELS:
            y = pe.labels_of(data.n_rows, mode)
            assert set(y) <= {-1, 1} and (mode in ("neg", "pos")) == (len(set(y)) == 1)
    # the blocks of `phases`: 64 rows and 641 hot slots each, so block b starts at slot phase b mod 8
    rows = pe.phases_rows()
    assert len(rows) == 8192
    for b in range(128):
        assert sum(h for h, _ in rows[64 * b:64 * b + 64]) == 641
        assert sum(max(c, 1) for _, c in rows[64 * b:64 * b + 64]) == sum(max(c, 1) for _, c in rows[:64])


@pytest.mark.parametrize("label_mode", ["mixed", "neg"])
def test_every_edge_class_is_reached_and_every_wrong_reader_is_caught(witness, tmp_path, label_mode):
    """(the tile shapes do not depend on the labels; the descriptors' low byte must not either: all -1 as well)"""
    totals, mutants = {}, {}
    for name in ("phases", "ragged"):
        totals[name], mutants[name], out = run_witness(witness, tmp_path, name, label_mode)
        assert out.count("RULE ") == 3
        assert totals[name]["max_slots"] <= 511
    assert totals["phases"]["max_slots"] == 511 and totals["phases"]["hot_nnz_mod_8"] == 0 and totals["ragged"]["hot_nnz_mod_8"] != 0
    for cls, names in CLASSES.items():
        for name in names:
            assert totals[name][cls] > 0, (cls, name, totals[name])
    for name in ("phases", "ragged"):
        assert mutants[name]["right"] == 0 and mutants[name]["mask_em_minus_1"] == 0, mutants[name]
        for m in WRONG_READERS:
            assert mutants[name][m] > 0, (m, name, mutants[name])
