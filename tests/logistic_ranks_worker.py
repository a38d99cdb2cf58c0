"""One rank of tests/test_gpu_logistic_ranks.py: an fp32 engine over its shard of the job's rows, attached with
comm_init_lg, running a scenario of tests/logistic_ranks_cases.py.  Over the tests' seam build and the stand-in collective
both ranks share device 0; with `--real` the product library over real RCCL, one device per rank.
usage: python logistic_ranks_worker.py <rank> <world> <workdir> <steps|cancel|widths|exact|mismatch> [--real]"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dsgd_amd  # noqa: E402
from dsgd_amd import _lib  # noqa: E402
from logistic_ranks_cases import rank_op, run_op, scenario  # noqa: E402
from world2_worker import exchange_uid  # noqa: E402


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def code_of(fn):
    try:
        fn()
    except _lib.DsgdError as e:
        return e.code
    return 0


def grid_weights(w):
    """w on the grid 2^-10, clipped to +-4: |w|^2 is then exact in fp64 whatever the order of the sum"""
    return (np.clip(np.rint(np.asarray(w, dtype=np.float64) * 1024.0), -4096, 4096) / 1024.0).astype(np.float32)


LOCAL_RANGES = [(0, 2048), (100, 4096)]


def local_probe(eng, w):
    """the three local calls on weights w: (gradient, [loss, acc] per range, probabilities)"""
    idx = np.random.default_rng(21).permutation(4096)[:300].astype(np.int32)
    g, st = eng.lg_gradient(idx, w=w)
    ev = np.asarray(eng.lg_loss_acc_ranges(LOCAL_RANGES, w=grid_weights(w)), dtype=np.float64)
    p = eng.lg_predict_proba(idx, w=w)
    return g, ev, p, np.asarray([st["n_samples"], st["n_active"]])


def uid(wd, name, rank):
    return exchange_uid(wd, name, rank, dsgd_amd.Engine.comm_unique_id)


def run_set(eng, s, rank, world, wd, tag, out, load=True):
    if load:
        eng.load_csr(*s["shards"][rank])
    eng.set_weights(s["w0"])
    eng.comm_init_lg(uid(wd, "uid_%s.bin" % tag, rank), world, rank)   # (loaded data: ranked again here, from the job's counts)
    out[tag + "__ranks"] = eng.column_ranks()
    w_hist, stats, kernels = [], [], []
    for op in s["ops"]:
        st, kern = run_op(eng, rank_op(op, rank))
        w_hist.append(eng.get_weights())
        stats.append(st)
        kernels.append(kern)
    out[tag + "__w_hist"] = np.stack(w_hist)
    out[tag + "__stats"] = np.asarray(stats)
    out[tag + "__kernels"] = np.asarray(kernels)


def run_steps(eng, s, rank, world, wd, out):
    # a column-slice plan from before the attach (its run is refused under the communicator)
    eng.load_csr(*s["shards"][rank])
    rng = np.random.default_rng(31 + rank)
    small = [[rng.permutation(4096)[:50].astype(np.int32) for _ in range(2)] for _ in range(2)]
    pre = eng.lg_plan(small, slices=True)
    run_set(eng, s, rank, world, wd, "synth", out, load=False)
    w = eng.get_weights()
    # local calls under the communicator: no collective (the ranks call them with different arguments' results in flight)
    g, ev, p, st = local_probe(eng, w)
    out["local_g"], out["local_eval"], out["local_p"], out["local_stats"] = g, ev, p, st
    eng.set_weights(w)
    # refusals: EUNSUPPORTED, the weights keep their bits
    split = [(0, 2048), (2048, 4096)]
    out["refused"] = np.asarray([code_of(lambda: eng.lg_plan_from_seed(12345, split, 2048, 100)),
                                 code_of(lambda: eng.lg_plan(small, slices=True)),
                                 code_of(lambda: eng.lg_plan_from_seed(12345, split, 2048, 100, slices=True)),
                                 code_of(lambda: eng.plan_run(pre, 0, 2, 0.5))])
    out["refused_w_same"] = np.asarray(np.array_equal(bits(w), bits(eng.get_weights())))
    # detached: a local step
    eng.comm_destroy()
    lists = [rng.permutation(4096)[:n].astype(np.int32) for n in (100, 37)]
    st = eng.lg_sync_step(lists, 0.5)
    out["w_local_from"], out["w_local"] = w, eng.get_weights()
    out["local_lists_0"], out["local_lists_1"] = lists
    out["stats_local"] = np.asarray([st["n_samples"], st["n_active"]])
    # the SVM's communicator: the logistic step stays refused
    eng.comm_init(uid(wd, "uid_plain.bin", rank), world, rank)
    out["plain_code"] = np.asarray(code_of(lambda: eng.lg_sync_step(lists, 0.5)))
    out["plain_w_same"] = np.asarray(np.array_equal(bits(out["w_local"]), bits(eng.get_weights())))
    eng.comm_destroy()
    pre.destroy()


def run_mismatch(eng, s, rank, world, wd, out):
    """rank r calls with 1 + r hosted workers: DSGD_EINVAL on every rank, nothing changed; the next agreed step runs"""
    eng.load_csr(*s["shards"][rank])
    eng.set_weights(s["w0"])
    eng.comm_init_lg(uid(wd, "uid_m.bin", rank), world, rank)
    rng = np.random.default_rng(300 + rank)
    lists = [rng.permutation(4096)[:200].astype(np.int32) for _ in range(1 + rank)]
    out["code"] = np.asarray(code_of(lambda: eng.lg_sync_step(lists, 0.5)))
    out["w_same"] = np.asarray(np.array_equal(bits(s["w0"]), bits(eng.get_weights())))
    flat = np.concatenate([lists[0], lists[0]])
    offs = np.asarray([0, 200, 400], dtype=np.int64)
    out["code_steps"] = np.asarray(code_of(lambda: eng.lg_sync_steps(flat[:200 * (2 - rank)], offs[:3 - rank], 2 - rank, 1, 0.5)))   # 2 steps against 1
    out["w_same_steps"] = np.asarray(np.array_equal(bits(s["w0"]), bits(eng.get_weights())))
    st = eng.lg_sync_step(lists[:1], 0.5)
    out["w_after"] = eng.get_weights()
    out["stats_after"] = np.asarray([st["n_samples"], st["n_active"]])
    eng.comm_destroy()


def main():
    rank, world, wd, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    real = "--real" in sys.argv
    if real:
        assert not os.environ.get("DSGD_LIB_PATH"), "the product library over real RCCL"
    else:
        assert os.environ.get("DSGD_RCCL_LIB"), "the worker must run with the shim selected explicitly"
        assert os.environ.get("DSGD_LIB_PATH", "").endswith("libdsgd_hip_seam.so"), "... through the tests' seam build of the library"
    out = {}
    sets = scenario("steps" if mode == "mismatch" else mode)
    for i, s in enumerate(sets):
        with dsgd_amd.Engine(s["dim"], s["lam"], device=rank if real else 0) as eng:
            if mode == "steps":
                run_steps(eng, s, rank, world, wd, out)
            elif mode == "mismatch":
                run_mismatch(eng, s, rank, world, wd, out)
            else:
                run_set(eng, s, rank, world, wd, "set%d" % i, out)
                eng.comm_destroy()
    np.savez(os.path.join(wd, "out_%d.npz" % rank), **out)
    print("rank %d done" % rank, flush=True)


if __name__ == "__main__":
    main()
