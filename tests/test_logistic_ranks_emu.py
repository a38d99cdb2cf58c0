"""CPU: the logistic step across ranks, emulated in numpy with tests/logistic_bound.py's emu_acc / emu_step (the kernels' own
operation order).  Two ranks: each fills its own workers' integer slots and length words of a zeroed buffer, the buffers are
added as int64 (the all-reduce), and every rank folds the K = k x world workers in global worker order at the common vexp.
That must be, bit for bit, emu_step on the concatenated data with the K lists -- and three mistakes must each change the bits
on the inputs of tests/logistic_ranks_cases.py: every rank quantising on its own vexp, the workers folded rank-minor, and a
worker's n taken from the local worker of the same number.  The swap of workers 0 and 3, which the GPU test uses as its
negative control, is shown not to commute here too."""

import numpy as np
import pytest

import logistic_bound as lb
from logistic_ranks_cases import LAM, LR, cancel_problem, concat, global_lists

WORLD, K_LOCAL = 2, 2
ROWS = 256   # per rank


def with_largest(csr, vmax):
    """the shard with one more row, never listed, that holds the job's largest value: vexp is a pure function of the largest
    |value|, so emu_acc on this shard quantises on the job's grid"""
    extra = (np.asarray([0, 1], np.int64), np.asarray([0], np.int32), np.asarray([vmax], np.float32), np.asarray([1], np.int8))
    return concat([csr, extra])


@pytest.fixture(scope="module")
def problem():
    job, shards, w, lists, F = cancel_problem(ROWS)
    return job, shards, w, lists


def ranks_step(shards, w, lists, mistake=None, reader=0):
    """the weights rank `reader` holds after the step"""
    dp = len(w)
    common = max(lb.vexp_of(s[2]) for s in shards)
    vmax = max(float(np.abs(s[2]).max()) for s in shards)
    K = K_LOCAL * WORLD
    total_slots, total_hdr = np.zeros((K, dp), dtype=np.int64), np.zeros(K, dtype=np.int64)
    for r in range(WORLD):
        slots, hdr = np.zeros((K, dp), dtype=np.int64), np.zeros(K, dtype=np.int64)   # this rank's buffer: zero but for its own workers
        data = shards[r] if mistake == "own_vexp" else with_largest(shards[r], vmax)
        for j, idx in enumerate(lists[r]):
            acc, S = lb.emu_acc(data, w, idx)
            assert S == lb.shift(len(idx))
            slots[r * K_LOCAL + j] = acc
            hdr[r * K_LOCAL + j] = len(idx)
        total_slots, total_hdr = total_slots + slots, total_hdr + hdr   # the all-reduce: an int64 sum
    wj = np.asarray(w, dtype=np.float32).astype(np.float64)
    reg = (2.0 * LAM) * wj
    total = np.zeros_like(wj)
    order = range(K)
    if mistake == "rank_minor":
        order = [r * K_LOCAL + j for j in range(K_LOCAL) for r in range(WORLD)]
    for g in order:
        n = len(lists[reader][g % K_LOCAL]) if mistake == "local_n" else int(total_hdr[g])
        Gk = total_slots[g].astype(np.float64) * 2.0 ** (common - lb.shift(n))
        total = total + (Gk + reg)
    mean = total / float(K)
    return (wj - float(np.float32(LR)) * mean).astype(np.float32)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def test_the_largest_value_lies_on_rank_1_only(problem):
    job, shards, w, lists = problem
    assert lb.vexp_of(shards[1][2]) == 40 and lb.vexp_of(shards[0][2]) <= 1
    assert lb.vexp_of(job[2]) == lb.vexp_of(with_largest(shards[0], float(np.abs(job[2]).max()))[2]) == 40
    assert [lb.shift(len(l)) for ls in lists for l in ls] == [55, 56, 53, 59]   # the same j: another shift on the other rank


def test_gather_and_fold_are_the_single_contexts_bits(problem):
    job, shards, w, lists = problem
    want = lb.emu_step(job, w, global_lists(lists, ROWS), LR, LAM)
    for reader in range(WORLD):
        assert np.array_equal(bits(ranks_step(shards, w, lists, reader=reader)), bits(want))
    assert np.count_nonzero(want != w) > 1000


@pytest.mark.parametrize("mistake", ["own_vexp", "rank_minor", "local_n"])
def test_each_mistake_changes_the_bits(problem, mistake):
    job, shards, w, lists = problem
    want = lb.emu_step(job, w, global_lists(lists, ROWS), LR, LAM)
    got = ranks_step(shards, w, lists, mistake=mistake)
    n = int(np.count_nonzero(bits(got) != bits(want)))
    print("%s: %d of %d weights differ" % (mistake, n, len(w)))
    assert n > 0


def test_swapping_workers_0_and_3_does_not_commute(problem):
    job, shards, w, lists = problem
    g = global_lists(lists, ROWS)
    a = lb.emu_step(job, w, g, LR, LAM)
    b = lb.emu_step(job, w, [g[3], g[1], g[2], g[0]], LR, LAM)
    assert not np.array_equal(bits(a), bits(b))
