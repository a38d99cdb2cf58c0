"""No GPU needed: the host's part of the device-drawn lists (csrc/dsgd_jr_walk.hpp) -- the epoch's frame, the walk over the
rejection candidates and the selection of the hosted workers' records -- as a program of its own under AddressSanitizer and
UBSan, against a draw-by-draw java.util.Random and against csrc/jrand.c.

The program makes the candidates the way dsgd_jr_scan_kernel's contract says (raw values >= 2^31 - longest split, cut into
per-workgroup blocks of 1024 * per_lane raw values, the blocks placed in a shuffled arrival order), runs frame and walk, and
computes the same records by stepping the LCG one raw value at a time through every shuffle with nextInt's own rejection
rule (`u - r + (bound - 1) < 0` in wrapping int arithmetic, not the walk's threshold form).

A job with a worker of ONE row runs one step whatever is asked for (the reference stops before a step in which any worker's
slice is empty), so the job of the six lengths is asked for 3 steps and has 1; the same job without that worker has the 3."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dsgd_amd import host

CSRC = os.path.join(ROOT, "distributed-sgd_amd", "csrc")
MULT, ADD, MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1
SEED = (20260 ^ MULT) & MASK   # (java.util.Random(20260)'s first state)

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dsgd_jr_walk.hpp"
typedef unsigned long long u64;
static u64 step(u64 s) { return (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1); }
static void print(const char* tag, const std::vector<JrShuf>& shuf, const std::vector<int>& rej) {
  for (size_t q = 0; q < shuf.size(); ++q) {
    std::printf("%s %zu %lld", tag, q, shuf[q].raw0);
    for (int i = shuf[q].rej_begin; i < shuf[q].rej_end; ++i) std::printf(" %d", rej[(size_t)i]);
    std::printf("\n");
  }
}
// argv: s0 first n_local batch max_samples exact len...   (exact: the first scan is `nominal` raw values long)
int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const u64 s0 = std::strtoull(argv[1], nullptr, 10);
  const int first = std::atoi(argv[2]), n_local = std::atoi(argv[3]), batch = std::atoi(argv[4]);
  const long long max_samples = std::atoll(argv[5]);
  const bool exact = std::atoi(argv[6]) != 0;
  std::vector<long long> len;
  long long max_len = 0;
  for (int i = 7; i < argc; ++i) {
    len.push_back(std::atoll(argv[i]));
    if (len.back() > max_len) max_len = len.back();
  }
  const long long n_steps = jr_epoch_steps(len, max_samples, batch);
  const JrFrame f = jr_frame(len, first, n_local, n_steps, batch);
  std::printf("frame %lld %lld %lld %lld\n", f.n_steps, f.n_shuf, f.n_lists, f.nominal);
  std::printf("offsets");
  for (size_t i = 0; i < f.offsets.size(); ++i) std::printf(" %lld", (long long)f.offsets[i]);
  std::printf("\n");
  // 1. the candidates of a scan, as the scan kernel delivers them
  const long long per_lane = 1024 < (1LL << 30) / max_len ? 1024 : (1LL << 30) / max_len, span = 1024 * per_lane;
  const unsigned int cand_min = (unsigned int)(0x80000000ULL - (u64)max_len);
  std::vector<long long> ci;
  std::vector<unsigned int> cu;
  std::vector<u64> base;
  auto scan_to = [&](long long scan) {
    const long long n_wg = (scan + span - 1) / span;
    std::vector<std::vector<long long>> bi((size_t)n_wg);
    std::vector<std::vector<unsigned int>> bu((size_t)n_wg);
    u64 s = s0;
    for (long long i = 0; i < scan; ++i) {
      s = step(s);
      const unsigned int u = (unsigned int)(s >> 17);
      if (u >= cand_min) {
        bi[(size_t)(i / span)].push_back(i);
        bu[(size_t)(i / span)].push_back(u);
      }
    }
    std::vector<long long> order((size_t)n_wg);   // the workgroups' arrival order: a Fisher-Yates of its own
    for (long long w = 0; w < n_wg; ++w) order[(size_t)w] = w;
    u64 x = 88172645463325252ULL;
    for (long long w = n_wg - 1; w > 0; --w) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      std::swap(order[(size_t)w], order[(size_t)(x % (u64)(w + 1))]);
    }
    ci.clear(), cu.clear(), base.assign((size_t)n_wg, 0);
    for (long long w : order) {
      if (bi[(size_t)w].size() > 8192) std::exit(3);
      base[(size_t)w] = ((u64)ci.size() << 16) | (u64)bi[(size_t)w].size();
      ci.insert(ci.end(), bi[(size_t)w].begin(), bi[(size_t)w].end());
      cu.insert(cu.end(), bu[(size_t)w].begin(), bu[(size_t)w].end());
    }
  };
  // 2. scan and walk, further where the walk says so
  JrWalked w;
  long long scan = exact ? f.nominal : f.nominal + 64 + f.nominal / 4096;
  for (int attempt = 0;; ++attempt) {
    scan_to(scan);
    if (jr_walk(f, len, JrCandidates{ci.data(), cu.data(), base.data(), (long long)base.size()}, scan, &w)) break;
    std::printf("outran %lld %lld\n", scan, w.scan_at_least);
    if (attempt >= 3) return 4;
    scan = w.scan_at_least + 64 + w.rej_total / 8;
  }
  std::printf("total %lld\n", w.rej_total);
  print("W", w.shuf, w.rej);
  // 3. the same records draw by draw
  std::vector<JrShuf> bs;
  std::vector<int> br;
  u64 s = s0;
  long long raw = 0;
  for (long long q = 0; q < f.n_shuf; ++q) {
    const long long raw0 = raw;
    const int begin = (int)br.size();
    for (int n = (int)len[(size_t)(q % (long long)len.size())]; n >= 2; --n)
      for (;;) {
        s = step(s);
        const int u = (int)(s >> 17), r = u % n;
        const long long off = raw++ - raw0;
        if ((n & (n - 1)) == 0 || (int)((unsigned int)u - (unsigned int)r + (unsigned int)(n - 1)) >= 0) break;
        br.push_back((int)off);
      }
    bs.push_back(JrShuf{raw0, begin, (int)br.size()});
  }
  std::printf("brute_total %lld\n", raw);
  print("B", bs, br);
  // the selection
  jr_select_hosted(f, &w);
  for (size_t q = 0; q < w.shuf.size(); ++q) std::printf("Srec %zu %lld %d %d\n", q, w.shuf[q].raw0, w.shuf[q].rej_begin, w.shuf[q].rej_end);
  print("S", w.shuf, w.rej);
  std::printf("selected_rej %zu\n", w.rej.size());
  return 0;
}
"""

L6 = (1 << 20, 3, 1, 2, (1 << 19) + 1, 65536)
#        name               lens                  first n_local batch max_samples exact
CASES = {"six_lengths":    (L6,                     0, 6, 1, 3, 0),
         "six_window":     (L6,                     1, 3, 1, 3, 0),
         "three_steps":    ((1 << 20, 3, (1 << 19) + 1, 65536), 0, 4, 1, 3, 0),
         "three_window":   ((1 << 20, 3, (1 << 19) + 1, 65536), 1, 2, 1, 3, 0),
         "one_worker_two": ((2,),                   0, 1, 1, 5, 0),
         "short_last":     ((10, 7),                0, 2, 4, 100, 0),
         "scan_is_nominal": (L6,                    0, 6, 1, 3, 1)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("jr_walk")
    src, exe = d / "jr_walk_test.cpp", d / "jr_walk_test"
    src.write_text(SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


_RUNS = {}


def run(program, name):
    """one run of the program per case, parsed once and left unchanged"""
    if name not in _RUNS:
        lens, first, n_local, batch, max_samples, exact = CASES[name]
        r = subprocess.run([program, str(SEED), str(first), str(n_local), str(batch), str(max_samples), str(exact)] + [str(x) for x in lens],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        out = {"W": [], "B": [], "S": [], "Srec": [], "outran": []}
        for line in r.stdout.splitlines():
            tag, *v = line.split()
            v = [int(x) for x in v]
            if tag in ("W", "B", "S"):
                assert v[0] == len(out[tag])
                out[tag].append((v[1], v[2:]))   # (raw0, the rejected offsets)
            elif tag in ("Srec", "outran"):
                out[tag].append(v)
            else:
                out[tag] = v
        _RUNS[name] = out
    return _RUNS[name]


def jump(s, n):
    a, c, ra, rc = MULT, ADD, 1, 0
    while n:
        if n & 1:
            ra, rc = (ra * a) & MASK, (rc * a + c) & MASK
        a, c = (a * a) & MASK, (c * a + c) & MASK
        n >>= 1
    return (s * ra + rc) & MASK


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_walk_is_the_stream_draw_by_draw(program, name):
    lens, first, n_local, batch, max_samples, exact = CASES[name]
    o = run(program, name)
    n_steps, n_shuf, n_lists, nominal = o["frame"]
    # the frame: the reference's rule for the steps, the lists' sizes
    want_steps = 0
    while want_steps * batch < max_samples and all(want_steps * batch < ln for ln in lens):
        want_steps += 1
    assert n_steps == want_steps and n_shuf == n_steps * len(lens) and n_lists == n_steps * n_local
    assert nominal == n_steps * sum(ln - 1 for ln in lens)
    sizes = [min(batch, lens[first + i] - s * batch) for s in range(n_steps) for i in range(n_local)]
    assert o["offsets"] == [0] + list(np.cumsum(sizes)) and min(sizes) >= 1
    # the walk against the draw-by-draw stream, record for record
    assert len(o["W"]) == len(o["B"]) == n_shuf
    for q, (w, b) in enumerate(zip(o["W"], o["B"])):
        assert w == b, (q, w, b)
    n_rej = sum(len(r) for _, r in o["W"])
    assert o["total"] == [n_rej] and o["brute_total"] == [nominal + n_rej]
    # the scan that was exactly `nominal` long had to be followed by a longer one
    assert (len(o["outran"]) >= 1) == bool(exact)
    for scan, need in o["outran"]:
        assert scan < need <= nominal + n_rej
    # the selection against picking the same records by hand
    rej_at, flat = 0, []
    assert len(o["S"]) == len(o["Srec"]) == n_lists
    for q in range(n_lists):
        raw0, rej = o["W"][(q // n_local) * len(lens) + first + q % n_local]
        assert o["S"][q] == (raw0, rej) and o["Srec"][q] == [q, raw0, rej_at, rej_at + len(rej)]
        rej_at += len(rej)
        flat += rej
    assert o["selected_rej"] == [len(flat)]


def test_the_cases_hold_what_they_are_for(program):
    o = run(program, "six_lengths")
    rej_of = {ln: len(o["W"][k][1]) for k, ln in enumerate(L6)}   # (one step: shuffle k is worker k's)
    assert o["frame"][0] == 1 and run(program, "three_steps")["frame"][0] == 3
    assert rej_of[1 << 20] > 64                        # more than dsgd_jr_slice_kernel's table holds
    assert rej_of[3] == 0                              # a shuffle with none
    assert o["W"][2][0] == o["W"][3][0]                # the worker of one row draws nothing: the next starts where it does
    assert rej_of[2] == 0                              # bound 2 alone: a power of two never rejects
    assert run(program, "scan_is_nominal")["W"] == o["W"]
    short = run(program, "short_last")
    assert short["offsets"] == [0, 4, 8, 12, 15]       # the last slice of the 7-row worker is 3 rows


@pytest.mark.parametrize("name", ["six_lengths", "three_steps", "short_last"])
def test_every_shuffle_starts_where_jrand_c_leaves_the_state(program, name):
    lens = CASES[name][0]
    o = run(program, name)
    lib = host._host_lib()
    assert lib is not None, "libdsgd_host.so is not built"
    starts = [raw0 for raw0, _ in o["W"]] + [o["brute_total"][0]]
    st = C.c_uint64(SEED)
    for q in range(len(o["W"])):
        ln = lens[q % len(lens)]
        assert st.value == jump(SEED, starts[q]), q
        buf = np.arange(ln, dtype=np.int32)
        used = int(lib.dsgd_jrand_shuffle(C.byref(st), buf.ctypes.data_as(C.c_void_p), C.c_int64(ln)))
        assert used == starts[q + 1] - starts[q] == (ln - 1 if ln > 1 else 0) + len(o["W"][q][1]), q
    assert st.value == jump(SEED, starts[-1])
