"""No GPU needed: rcv1.load_topics against a pure-Python restatement, on a folder rcv1.export wrote with extra qrels lines.
The planes follow the multi-label rule (+1 iff ANY line tags the document), `load` keeps the reference's last-line rule."""

import os

import numpy as np
import pytest

import dsgd_amd
from dsgd_amd import rcv1

TOPICS = ["CCAT", "GCAT", "ECAT", "MCAT", "E11"]          # E11: no line names it


def planes_ref(folder, topics, ids):
    tags = {}
    for line in open(os.path.join(folder, rcv1.QRELS)).read().splitlines():
        parts = line.split(" ")
        tags.setdefault(int(parts[1]), set()).add(parts[0])
    return np.array([[1 if t in tags.get(int(i), ()) else -1 for i in ids] for t in topics], dtype=np.int8)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rcv1_topics"))
    data = dsgd_amd.synth.generate(60, seed=5)
    ids = rcv1.export(path, data, n_train_file=40)
    with open(os.path.join(path, rcv1.QRELS), "a") as f:
        f.write("GCAT %d 1\n" % ids[1])                  # a CCAT document tagged GCAT afterwards
        f.write("GCAT 999999 1\nCCAT 999998 1\n")        # ids no row carries
        f.write("MCAT %d 1\nMCAT %d 1\n" % (ids[2], ids[2]))   # the same tag twice
    return path, data, ids


def test_planes_follow_the_any_line_rule(folder):
    path, data, ids = folder
    got, planes = rcv1.load_topics(path, TOPICS)
    want, want_ids = rcv1.load(path, with_ids=True)
    assert np.array_equal(want_ids, ids)
    for a, b in ((got.row_ptr, want.row_ptr), (got.col, want.col), (got.val, want.val), (got.label, want.label), (got.val64, want.val64)):
        assert np.array_equal(a, b)                       # load's rows, its labels included
    assert planes.dtype == np.int8 and planes.shape == (len(TOPICS), 60) and planes.flags.c_contiguous
    assert np.array_equal(planes, planes_ref(path, TOPICS, ids))
    assert set(np.unique(planes)) <= {-1, 1}
    ccat, gcat = planes[0], planes[1]
    both = np.where((ccat == 1) & (gcat == 1))[0]
    assert len(both) > 0 and np.all(want.label[both] == -1)          # CCAT then GCAT: +1 on both planes, -1 for load
    assert np.all(ccat[want.label == 1] == 1)                        # what load calls +1 carries a CCAT line (its last one)
    assert planes[3][2] == 1 and want.label[2] == -1                 # row 2: MCAT appended twice -- one tag here, the last line for load
    assert np.all(planes[4] == -1)                                   # an untagged topic
    assert np.array_equal(rcv1.load_topics(path, "GCAT")[1], planes[1:2])
    train_only, p_train = rcv1.load_topics(path, TOPICS, full=False)
    assert train_only.n_rows == 40 and np.array_equal(p_train, planes[:, :40])
    twice = rcv1.load_topics(path, ["GCAT", "GCAT"])[1]              # a topic listed twice: two equal planes
    assert np.array_equal(twice[0], planes[1]) and np.array_equal(twice[1], planes[1])


def test_refusals(folder, tmp_path):
    path, data, ids = folder
    for bad in ([], ["A"] * 65, [""], ["C CAT"], [5]):
        with pytest.raises(ValueError):
            rcv1.load_topics(path, bad)
    with pytest.raises(ValueError):
        rcv1.load_topics(str(tmp_path / "nowhere"), ["CCAT"])
    # an unknown id: a document no qrels line names makes load raise, as in the reference
    other = str(tmp_path / "unlabelled")
    rcv1.export(other, data, n_train_file=40)
    with open(os.path.join(other, rcv1.FILES[0]), "a") as f:
        f.write("777777  1:0.5\n")
    with pytest.raises(ValueError, match="no label"):
        rcv1.load_topics(other, ["CCAT"])
    with open(os.path.join(other, rcv1.QRELS), "a") as f:
        f.write("GCAT 777777 1\nCCAT notanumber 1\n")
    with pytest.raises(ValueError, match="malformed"):
        rcv1.load_topics(other, ["CCAT"])
