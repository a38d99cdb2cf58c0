"""-m gpu: host.MasterSync under DSGD_DEVICE_LISTS_JOB=1 -- where the device draw of an epoch's lists is refused
(DSGD_EUNSUPPORTED: here a batch of 2,500 rows) the job form (Engine.plan_from_seed_job) is tried before the host's
generator, and the fit is bit for bit the fit on the host's lists (DSGD_DEVICE_LISTS=0): weights, losses per epoch, the
generator's state, the steps run.  Without the knob the calls are those of today: the refused draw, then the host."""

import numpy as np
import pytest

import dsgd_amd
from conftest import has_gpu
from dsgd_amd import host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="no gfx950 device")]

LAM = 1e-5
N_ROWS, N_TRAIN = 23149, 18519
BATCH, EPOCHS, NODES = 2500, 2, 3      # splits of 6,173 rows: 3 steps an epoch, the last of 1,173 rows per worker


class Recorder:
    """the engine behind the backend interface: which list-drawing calls were made and what became of them"""

    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def _record(self, name, fn, *a, **kw):
        tag = name + ("(rp64)" if kw.get("rp64") else "")
        try:
            out = fn(*a, **kw)
        except dsgd_amd.DsgdError as e:
            self.calls.append((tag, e.code))
            raise
        self.calls.append((tag, 0))
        return out

    def plan_from_seed(self, *a, **kw):
        return self._record("plan_from_seed", self.eng.plan_from_seed, *a, **kw)

    def plan_from_seed_job(self, *a, **kw):
        return self._record("plan_from_seed_job", self.eng.plan_from_seed_job, *a, **kw)

    def plan_flat(self, *a, **kw):
        return self._record("plan_flat", self.eng.plan_flat, *a, **kw)

    def __getattr__(self, name):
        return getattr(self.eng, name)


@pytest.fixture(scope="module")
def data():
    return dsgd_amd.synth.generate(N_ROWS, seed=3)


def _fit(eng, data, monkeypatch, device_lists, job):
    monkeypatch.setenv("DSGD_DEVICE_LISTS_MIN_DRAWS", "1")
    monkeypatch.setenv("DSGD_DEVICE_LISTS", "1" if device_lists else "0")
    if job:
        monkeypatch.setenv("DSGD_DEVICE_LISTS_JOB", "1")
    else:
        monkeypatch.delenv("DSGD_DEVICE_LISTS_JOB", raising=False)
    backend = Recorder(eng)
    m = host.MasterSync(backend, N_TRAIN, N_ROWS, node_count=NODES, rnd=host.JavaRandom(0), plans=True)
    s = m.fit(np.zeros(data.dim + 1), EPOCHS, BATCH, 0.5, lambda losses: False)
    w = eng.get_weights()
    return {"w": w.view(np.uint8).copy(), "grad": np.array(s.grad).view(np.uint8).copy(), "seed": m.rnd.seed, "steps": m.steps_run,
            "losses": list(m.losses), "test_losses": list(m.test_losses), "accs": list(m.accs)}, backend.calls


def _same(a, b):
    assert a["steps"] == b["steps"] == EPOCHS * 3 and a["seed"] == b["seed"] != host.JavaRandom(0).seed
    assert len(a["losses"]) == EPOCHS and a["losses"] == b["losses"] and a["test_losses"] == b["test_losses"] and a["accs"] == b["accs"]
    assert np.array_equal(a["w"], b["w"]) and np.array_equal(a["grad"], b["grad"]) and a["w"].any()


def test_fp32_fit_through_the_job_form_is_the_fit_on_the_hosts_lists(data, monkeypatch):
    with dsgd_amd.Engine(data.dim, LAM) as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(N_TRAIN)
        on_host, calls_host = _fit(eng, data, monkeypatch, device_lists=False, job=False)
        today, calls_today = _fit(eng, data, monkeypatch, device_lists=True, job=False)
        by_job, calls_job = _fit(eng, data, monkeypatch, device_lists=True, job=True)
    _same(by_job, on_host)
    _same(today, on_host)
    # the job form was called and not refused: once per epoch drawn (fit draws the epoch after the last ahead and puts it back)
    jobs = [c for c in calls_job if c[0] == "plan_from_seed_job"]
    assert len(jobs) >= EPOCHS and all(code == 0 for _, code in jobs)
    assert calls_job[0] == ("plan_from_seed", -7) and calls_job[1] == ("plan_from_seed_job", 0)
    assert [c for c in calls_job if c[0] == "plan_from_seed"] == [("plan_from_seed", -7)]   # (the refused form is not asked again)
    assert not any(c[0].startswith("plan_flat") for c in calls_job)                          # ... and the host drew nothing
    # without the knob: the refused draw, then the host's lists -- no job form
    assert calls_today[0] == ("plan_from_seed", -7) and not any("job" in c[0] for c in calls_today + calls_host)
    assert [c for c in calls_today[1:] if c[0] != "plan_flat"] == [] and len(calls_today) >= 1 + EPOCHS
    assert all(c[0] == "plan_flat" and c[1] == 0 for c in calls_host) and len(calls_host) >= EPOCHS


def test_fp64_fit_through_the_job_form_is_the_fit_on_the_hosts_lists(data, monkeypatch):
    """DSGD_F64_RP_PLANS=1: the column-slice forms refuse 2,500 rows per step, plan_from_seed(rp64=True) refuses the batch, the
    job form draws the row-parallel plan"""
    monkeypatch.setenv("DSGD_F64_RP_PLANS", "1")
    with dsgd_amd.Engine(data.dim, LAM, precision="fp64") as eng:
        eng.load_csr(data.row_ptr, data.col, data.val, data.label)
        eng.build_dim_sparsity(N_TRAIN)
        on_host, calls_host = _fit(eng, data, monkeypatch, device_lists=False, job=False)
        today, calls_today = _fit(eng, data, monkeypatch, device_lists=True, job=False)
        by_job, calls_job = _fit(eng, data, monkeypatch, device_lists=True, job=True)
    _same(by_job, on_host)
    _same(today, on_host)
    jobs = [c for c in calls_job if c[0] == "plan_from_seed_job(rp64)"]
    assert len(jobs) >= EPOCHS and all(code == 0 for _, code in jobs)
    assert ("plan_from_seed(rp64)", -7) in calls_job and calls_job.index(("plan_from_seed(rp64)", -7)) < calls_job.index(jobs[0])
    assert [c for c in calls_job if c[0] == "plan_from_seed(rp64)"] == [("plan_from_seed(rp64)", -7)]
    assert not any(c[0] == "plan_flat(rp64)" for c in calls_job)
    # without the knob the row-parallel plans are made of the host's lists, as today
    assert not any("job" in c[0] for c in calls_today + calls_host)
    assert ("plan_from_seed(rp64)", -7) in calls_today and sum(1 for c in calls_today if c == ("plan_flat(rp64)", 0)) >= EPOCHS
    assert sum(1 for c in calls_host if c == ("plan_flat(rp64)", 0)) >= EPOCHS
