"""No GPU needed: the packed copies of the split streams that the row-chunk kernel's PACKED form reads (csrc/dsgd_fstep.hpp;
DSGD_FSTEP_PACKED) -- hot rank words with the row starts in bit 15, values folded with their row's label.

csrc/dsgd_layout_host.hpp states the construction (packed_streams_ref: what dsgd_pack_streams_kernel builds) and the way the
kernel turns a lane's eight flags back into start bits (packed_lane_bits: window rounded up to 8 slots, the end mark set by
the reader, starts of earlier rows in front of the tile's first row dropped).  tests/cpp/packed_streams_test.cpp, compiled with
AddressSanitizer and UBSan and run as a program of its own, holds those bits to the low byte of the lane descriptors that
wave_tile_meta writes -- for every tile of build_wave_tiles and of cut_row_chunks' tables, lane by lane -- and the folded
values to label x value, on row lengths 1, 7, 8, 9, 503, 504, tiles whose slot count is a multiple of 8 (also at the end of
the stream), windows that open on the starts of earlier rows, emptied and long rows between tiled rows and at the end, more
than 64 rows in a tile, the 254-row cap, and labels that are all -1.  The program insists that each of these was met."""

import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")


def test_packed_streams_under_sanitizers(tmp_path):
    exe = str(tmp_path / "packed_streams_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "packed_streams_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "all checks passed" in r.stderr
