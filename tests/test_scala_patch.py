"""The reference-side patch (scala/patch/dsgd-hip-backend.diff) must keep applying, so it cannot rot silently.  The
upstream tree is not part of this repository, so the test rebuilds from the diff itself the part of every file it
modifies that the diff shows -- each hunk's context and removed lines at the line numbers its header names, one distinct
placeholder line everywhere else -- and applies the patch to that skeleton, dry run first and then for real: every hunk
must be well formed and apply at its stated line with no fuzz and no offset.  (No JVM here: whether it COMPILES is for a
maintainer with sbt; what this pins as well is that the patch touches exactly the seams INTEGRATION.md names, that the
file it adds is scala/NativeSVM.scala byte for byte, and that every @native the patched code can reach is exported by
the JNI shim -- tests/test_jni_shim.py compares those two lists.)"""

import os
import re
import subprocess

from conftest import ROOT

PATCH = os.path.join(ROOT, "scala", "patch", "dsgd-hip-backend.diff")


def pre_image_skeletons(text):
    """{path: lines} of every file the diff modifies (not the one it adds): the lines its hunks expect, at their lines"""
    files, path, pos = {}, None, None
    for line in text.splitlines():
        if line.startswith("diff "):
            path, pos = None, None
        elif line.startswith("--- a/"):
            path = line[len("--- a/"):].split("\t")[0]
        elif line.startswith("@@ ") and path:
            m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", line)
            assert m, line
            pos = int(m.group(1))
            if pos == 0:       # a file the patch creates: nothing to rebuild
                path = None
                continue
            files.setdefault(path, {})
        elif path and pos is not None and line[:1] in (" ", "-"):
            assert files[path].setdefault(pos, line[1:]) == line[1:], (path, pos)   # two hunks disagree about a line
            pos += 1
    return {p: [lines.get(i, "// placeholder for upstream line %d of %s" % (i, p)) for i in range(1, max(lines) + 1)]
            for p, lines in files.items()}


def test_patch_applies_to_its_pre_image(tmp_path):
    tree = tmp_path / "ref"
    for path, lines in pre_image_skeletons(open(PATCH).read()).items():
        (tree / path).parent.mkdir(parents=True, exist_ok=True)
        (tree / path).write_text("\n".join(lines) + "\n")
    dry = subprocess.run(["patch", "-p1", "--dry-run", "-i", PATCH], cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert dry.returncode == 0 and "FAILED" not in dry.stdout and "fuzz" not in dry.stdout and "offset" not in dry.stdout, dry.stdout
    real = subprocess.run(["patch", "-p1", "-i", PATCH], cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert real.returncode == 0, real.stdout
    touched = sorted(re.findall(r"patching file (\S+)", real.stdout))
    base = "src/main/scala/epfl/distributed/"
    assert touched == sorted(["src/main/resources/application.conf", base + "Main.scala", base + "utils/Config.scala",
                              base + "core/Slave.scala", base + "core/Master.scala", base + "core/MasterAsync.scala",
                              base + "core/ml/NativeSVM.scala"])
    added = (tree / base / "core/ml/NativeSVM.scala").read_text()
    assert added == open(os.path.join(ROOT, "scala", "NativeSVM.scala")).read()
    # the seams of INTEGRATION.md, each behind `dsgd.backend = hip` with the JVM path left as it was
    slave = (tree / base / "core/Slave.scala").read_text()
    master = (tree / base / "core/Master.scala").read_text()
    masync = (tree / base / "core/MasterAsync.scala").read_text()
    main = (tree / base / "Main.scala").read_text()
    conf = (tree / "src/main/resources/application.conf").read_text()
    assert "backend = jvm" in conf and "${?DSGD_BACKEND}" in conf
    assert 'backend: String = "jvm"' in (tree / base / "utils/Config.scala").read_text()
    assert "new HipSVM(config.lambda, dimSparsity, data, trainData.length)" in main and "new SparseSVM(config.lambda, dimSparsity)" in main
    for call in ("h.gradientBatch(w, samplesIdx)", "h.forwardBatch(w, samplesIdx)", "h.asyncStepBatch(sampleIdx, learningRate)",
                 "h.updateGrad(request.gradUpdate)", "h.setWeights(request.weights)"):
        assert call in slave, call
    assert "model.backward(w, x, y)" in slave and "model.regularize(grad, w)" in slave      # the JVM bodies are still there
    # the resident (dev) master hands a whole EPOCH over as one plan: the lists drawn first, in the reference's own order
    assert "h.fitEpoch(batches, learningRate)" in master and "worker.gradient(req)" in master
    assert "split.map(Random.shuffle(_)).toSeq.take(nWorkers).map(_.slice(batch, batch + batchSize))" in master
    assert master.count("split.map(Random.shuffle(_))") == 2      # ... and the per-request loop still draws them itself
    assert 'Kamon.timer("master.sync.batch.duration").record(perBatch)' in master
    assert "h.lossAndAccuracy(weights, lo, hi)" in master
    # resident (dev) mode: the loss check evaluates the device weights in place -- a snapshot written back would discard
    # the updates the slave threads applied since it was taken
    assert "NativeSVM.lossAcc(ctx, if (resident) null else DenseKeys.fromVec(w), rowBegin, rowEnd, out)" in added
    assert "HipSVM.isResident(model)" in masync and "_.update(request.gradUpdate)" in masync
    # every method the patched code calls on HipSVM exists in the file the patch adds
    used = set(re.findall(r"\bh\.(\w+)\(", slave + master + masync + main)) | {"weights"}
    defined = set(re.findall(r"def (\w+)\(", added)) | set(re.findall(r"var (\w+)\s*:", added))
    assert used <= defined | {"resident"}, used - defined


def test_patch_is_a_plain_unified_diff():
    text = open(PATCH).read()
    assert text.count("\ndiff -ruN ") + text.startswith("diff -ruN ") == 7
    assert "/root/" not in text and "/tmp/" not in text      # relative a/ b/ paths only: applies with -p1 anywhere
