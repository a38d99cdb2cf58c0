package epfl.distributed.core.ml

import epfl.distributed.math.Vec
import spire.math.Number

/** JVM face of libdsgd_hip (include/dsgd.h) -- the binding a maintainer of zifeo/distributed-sgd adds.
  *
  * `SparseSVM` keeps its constructor and its six methods (core/ml/SparseSVM.scala:11-31); `HipSVM` below is a
  * subclass whose batch-level entry points replace the bodies of `SlaveImpl.gradient` / `forward`
  * (core/Slave.scala:129-157), of the `Slave.asyncTask` iteration and `updateGrad` (core/Slave.scala:79-111,177-185), of
  * `Master.localLoss` / `localAccuracy` (core/Master.scala:100-107) and of the `Master.fit` batch closure
  * (core/Master.scala:179-199) -- a whole epoch of it as ONE resident plan (`fitEpoch`) -- when `dsgd.backend = hip` (a new
  * OPTIONAL key; every existing `dsgd { ... }` key of
  * application.conf is untouched).  scala/patch/dsgd-hip-backend.diff is the patch that wires it in (it adds this file
  * as src/main/scala/epfl/distributed/core/ml/NativeSVM.scala).
  */
object NativeSVM {
  // The natives live on the module class `NativeSVM$`: their JNI names are
  // Java_epfl_distributed_core_ml_NativeSVM_00024_<name>(JNIEnv*, jobject self, ...) -- jni/dsgd_jni.cpp exports
  // exactly these (tests/test_jni_shim.py compares the two lists).
  System.loadLibrary("dsgd_jni") // jni/dsgd_jni.cpp, links libdsgd_hip.so

  @native def create(nFeatures: Int, lambda: Double, device: Int): Long
  @native def destroy(ctx: Long): Unit
  // the fp64 mode (include/dsgd.h "THE FP64 MODE"): Double weights and learning rate, the reference's own trajectory
  @native def createF64(nFeatures: Int, lambda: Double, device: Int): Long
  @native def setWeightsF64(ctx: Long, w: Array[Double]): Unit
  @native def getWeightsF64(ctx: Long, wOut: Array[Double]): Unit
  @native def planRunF64(ctx: Long, plan: Long, stepBegin: Long, stepEnd: Long, lr: Double): Unit
  @native def loadCsr(ctx: Long, rowPtr: Array[Long], col: Array[Int], value: Array[Float], label: Array[Byte]): Unit
  // an fp64 context only: the values as the Vec holds them (utils/Dataset.scala:30 reads Doubles), no rounding to Float
  @native def loadCsrF64(ctx: Long, rowPtr: Array[Long], col: Array[Int], value: Array[Double], label: Array[Byte]): Unit
  @native def buildDimSparsity(ctx: Long, nTrain: Long): Unit
  @native def gradient(ctx: Long, w: Array[Float], idx: Array[Int], gOut: Array[Float]): Long
  @native def forward(ctx: Long, w: Array[Float], idx: Array[Int], predOut: Array[Float]): Unit
  @native def syncStep(ctx: Long, idxPerWorker: Array[Array[Int]], lr: Float): Long
  @native def syncStepRanges(ctx: Long, rowBegin: Array[Long], rowEnd: Array[Long], lr: Float): Long
  // an epoch of Master.fit as ONE resident plan (core/Master.scala:179-199): idx = the epoch's lists concatenated
  // (batch-major, worker-minor), offsets = nSteps * nWorkers + 1 prefix offsets
  @native def planCreate(ctx: Long, idx: Array[Int], offsets: Array[Long], nWorkers: Int): Long
  @native def planCreateFromSeed(ctx: Long, state: Array[Long], splitBegin: Array[Long], splitEnd: Array[Long], maxSamples: Long, batchSize: Int): Long
  // row-parallel plans of an fp64 context (include/dsgd.h "THE FP64 MODE", ROW-PARALLEL PLANS): the twins' arguments; what the
  // creators above refuse there -- Double values, > 4 workers, > 1,024 rows per batch, a model beyond a slice's LDS
  @native def planCreateRp64(ctx: Long, idx: Array[Int], offsets: Array[Long], nWorkers: Int): Long
  @native def planCreateFromSeedRp64(ctx: Long, state: Array[Long], splitBegin: Array[Long], splitEnd: Array[Long], maxSamples: Long, batchSize: Int): Long
  // the same epoch for a JOB's share of workers (dsgd_plan_create_from_seed_job / _rp64): the stream over all jobLen.length workers, the lists of
  // the splitBegin.length hosted here (job workers first ..); any batch size, usable with a communicator attached; state as planCreateFromSeed
  @native def planCreateFromSeedJob(ctx: Long, state: Array[Long], jobLen: Array[Long], first: Int, splitBegin: Array[Long], maxSamples: Long, batchSize: Int, rp64: Boolean): Long
  // updates [firstUpdate, firstUpdate + nUpdates) of the zero-lag asynchronous schedule, the lists drawn by the device
  @native def asyncPlanCreateRp64(ctx: Long, assignedBegin: Array[Long], assignedEnd: Array[Long], batch: Int, seed: Long,
                                  positionalBug: Boolean, firstUpdate: Long, nUpdates: Long): Long
  @native def planRun(ctx: Long, plan: Long, stepBegin: Long, stepEnd: Long, lr: Float): Unit
  @native def planSynchronize(ctx: Long): Long
  @native def planDestroy(ctx: Long, plan: Long): Unit
  @native def lossAcc(ctx: Long, w: Array[Float], rowBegin: Long, rowEnd: Long, out: Array[Double]): Unit
  // Master.predict / distributedLoss / distributedAccuracy (core/Master.scala:61-98) in one launch: range k = worker k's split;
  // predOut: one byte in {-1, 0, +1} per row, range-major; out = {loss, accuracy}; w null = the resident weights
  @native def predictRanges(ctx: Long, w: Array[Float], rowBegin: Array[Long], rowEnd: Array[Long], predOut: Array[Byte], out: Array[Double]): Unit
  // Master.localSampledLoss / localSampledAccuracy (core/Master.scala:109-118) in one launch: over the rows idx names (lossAccList,
  // out = {loss, accuracy}), or over a sample the device draws from java.util.Random's 48-bit state (lossAccSampled: returns the
  // state behind the shuffle; out = {loss, accuracy, rows evaluated, raw values drawn}; UnsupportedOperationException beyond the
  // device form's limits, nothing drawn); w null = the resident weights
  @native def lossAccList(ctx: Long, w: Array[Float], idx: Array[Int], out: Array[Double]): Unit
  @native def lossAccSampled(ctx: Long, w: Array[Float], state: Long, rowBegin: Long, rowEnd: Long, samplesCount: Long, out: Array[Double]): Long
  @native def asyncStep(ctx: Long, idx: Array[Int], lr: Float, deltaOut: Array[Float]): Unit
  @native def updateGrad(ctx: Long, keys: Array[Int], values: Array[Float]): Unit
  // the same in the fp64 mode: Double learning rate, delta (D+1) and values
  @native def asyncStepF64(ctx: Long, idx: Array[Int], lr: Double, deltaOut: Array[Double]): Unit
  @native def updateGradF64(ctx: Long, keys: Array[Int], values: Array[Double]): Unit
  // SlaveImpl.gradient / forward in Double: w may be null (the resident weights); gradientF64 returns the active rows
  @native def gradientF64(ctx: Long, w: Array[Double], idx: Array[Int], gOut: Array[Double]): Long
  @native def forwardF64(ctx: Long, w: Array[Double], idx: Array[Int], predOut: Array[Double]): Unit
  // an epoch's steps of the fp64 mode in ONE call (dsgd_sync_steps_f64: planCreate's flat lists, the bits of one step call each; what
  // the plans refuse -- Double values, > 4 workers, > 1,024 rows per step); activeOut: null or one Long per step; returns the active rows
  @native def syncStepsF64(ctx: Long, idx: Array[Int], offsets: Array[Long], nWorkers: Int, lr: Double, activeOut: Array[Long]): Long
  // Sparse values (include/dsgd.h "SPARSE VALUES"): a Vec's map crosses as (keys, values).  A producing native compacts into
  // native scratch of D + 1 slots the shim owns per context and returns the number of pairs; takeSparse copies them into
  // arrays of exactly that length (hold the model's monitor across the two calls).  wKeys / wVals null: the resident weights.
  @native def gradientSparse(ctx: Long, wKeys: Array[Int], wVals: Array[Float], idx: Array[Int], statsOut: Array[Long]): Int
  @native def gradientSparseF64(ctx: Long, wKeys: Array[Int], wVals: Array[Double], idx: Array[Int], statsOut: Array[Long]): Int
  @native def asyncStepSparse(ctx: Long, idx: Array[Int], lr: Float): Int
  @native def asyncStepSparseF64(ctx: Long, idx: Array[Int], lr: Double): Int
  @native def getWeightsSparse(ctx: Long): Int
  @native def getWeightsSparseF64(ctx: Long): Int
  @native def setWeightsSparse(ctx: Long, keys: Array[Int], vals: Array[Float]): Unit
  @native def setWeightsSparseF64(ctx: Long, keys: Array[Int], vals: Array[Double]): Unit
  @native def takeSparse(ctx: Long, keysOut: Array[Int], valsOut: Array[Float]): Unit
  @native def takeSparseF64(ctx: Long, keysOut: Array[Int], valsOut: Array[Double]): Unit
  @native def asyncStart(ctx: Long, assignedBegin: Array[Long], assignedEnd: Array[Long], batch: Int, lr: Float,
                         maxUpdates: Long, seed: Long, positionalBug: Boolean): Unit
  @native def asyncUpdates(ctx: Long): Long
  @native def asyncStop(ctx: Long): Unit
  @native def asyncWait(ctx: Long): Unit
  @native def setWeights(ctx: Long, w: Array[Float]): Unit
  @native def getWeights(ctx: Long, wOut: Array[Float]): Unit
  // one process per GPU in the fp64 mode: rank 0 fills idOut (128 bytes) and hands it to the other ranks; every rank attaches
  // its fp64 context with it -- from then on syncStep / lossAcc span the ranks, bit for bit one process over all the rows
  @native def commUniqueId(idOut: Array[Byte]): Unit
  @native def commInitF64(ctx: Long, uniqueId: Array[Byte], worldSize: Int, rank: Int): Unit
  // the same on Double feature values (loadCsrF64): both words of every column sum travel; float data: exactly commInitF64
  @native def commInitF64v(ctx: Long, uniqueId: Array[Byte], worldSize: Int, rank: Int): Unit
  @native def commDestroy(ctx: Long): Unit
  // several GPUs driven by ONE thread of this JVM (dev role: master + every slave in one JVM, Main.scala:144-158): one
  // context per device, rank i = ctxs(i); arrays over workers are context-major (include/dsgd.h, dsgd_*_devices)
  @native def commInitAll(ctxs: Array[Long]): Unit
  @native def buildDimSparsityDevices(ctxs: Array[Long], nTrain: Array[Long]): Unit
  @native def syncStepDevices(ctxs: Array[Long], idxPerWorker: Array[Array[Int]], workersPerCtx: Int, lr: Float): Long
  @native def syncStepRangesDevices(ctxs: Array[Long], rowBegin: Array[Long], rowEnd: Array[Long], workersPerCtx: Int, lr: Float): Long
  @native def lossAccDevices(ctxs: Array[Long], rowBegin: Array[Long], rowEnd: Array[Long], out: Array[Double]): Unit
}

/** Dense float[D+1] indexed by KEY is the exchange format: feature ids are 1-based map keys
  * (utils/Dataset.scala:30), dimSparsity uses 0-based keys (Main.scala:60-62), so both slot 0 and slot D exist. */
/** A Vec's map as the (keys, values) pairs the sparse natives take and return: nothing of D + 1 slots is built or scanned. */
object SparsePairs {
  def fromVec(v: Vec): (Array[Int], Array[Float]) = {
    val n    = v.map.size
    val keys = new Array[Int](n)
    val vals = new Array[Float](n)
    var i    = 0
    v.map.foreach { case (k, x) => keys(i) = k; vals(i) = x.toDouble.toFloat; i += 1 }
    (keys, vals)
  }
  def toVec(keys: Array[Int], vals: Array[Float], size: Int): Vec = {
    val b = Map.newBuilder[Int, Number]
    b.sizeHint(keys.length)
    var i = 0
    while (i < keys.length) { b += keys(i) -> Number(vals(i).toDouble); i += 1 }
    Vec(b.result(), size)
  }
}

object DenseKeys {
  def fromVec(v: Vec): Array[Float] = {
    val a = new Array[Float](v.size + 1)
    v.map.foreach { case (k, n) => a(k) = n.toDouble.toFloat }
    a
  }
  def toVec(a: Array[Float], size: Int): Vec =
    Vec(a.iterator.zipWithIndex.collect { case (x, k) if x != 0f => k -> Number(x.toDouble) }.toMap, size)
}

class HipSVM(lambda: Number, dimSparsity: Vec, data: Array[(Vec, Int)], nTrain: Int, device: Int = 0)
    extends SparseSVM(lambda, dimSparsity) {

  private val dim = data(0)._1.size
  // -Ddsgd.precision=fp64: an fp64 context that is given the Vec values as they are (INTEGRATION.md 3a)
  private val fp64 = sys.props.get("dsgd.precision").contains("fp64")
  // -Ddsgd.f64.rpPlans=true (fp64 only; off by default, DESIGN.md 3.8): an epoch whose plan the column slices refuse runs
  // as a resident row-parallel plan (planCreateRp64 / planCreateFromSeedRp64) instead of failing
  private val rpPlans = fp64 && sys.props.get("dsgd.f64.rpPlans").contains("true")
  private def refused(e: RuntimeException): Boolean =
    rpPlans && !e.isInstanceOf[IllegalArgumentException] && !e.isInstanceOf[IndexOutOfBoundsException]
  private val ctx =
    if (fp64) NativeSVM.createF64(dim, lambda.toDouble, device) else NativeSVM.create(dim, lambda.toDouble, device)

  {
    // Array[(Vec, Int)] -> CSR, columns ascending (the order of the text files, utils/Dataset.scala:19-34)
    val rowPtr = new Array[Long](data.length + 1)
    val cols   = Array.newBuilder[Int]
    val vals   = Array.newBuilder[Double]
    val labels = new Array[Byte](data.length)
    var nnz    = 0L
    data.zipWithIndex.foreach {
      case ((x, y), i) =>
        x.map.toSeq.sortBy(_._1).foreach { case (k, n) => cols += k; vals += n.toDouble; nnz += 1 }
        rowPtr(i + 1) = nnz
        labels(i) = y.toByte
    }
    if (fp64) NativeSVM.loadCsrF64(ctx, rowPtr, cols.result(), vals.result(), labels)
    else NativeSVM.loadCsr(ctx, rowPtr, cols.result(), vals.result().map(_.toFloat), labels)
    NativeSVM.buildDimSparsity(ctx, nTrain)
  }

  /** one process per GPU (INTEGRATION.md 3b): this worker's context joins the job's communicator -- `uniqueId` is rank 0's
    * NativeSVM.commUniqueId, handed over any host channel.  An fp64 context always holds Doubles (loadCsrF64 above), so it
    * attaches through commInitF64v; from then on syncStep / lossAcc span the ranks, bit for bit one process over all rows. */
  def attachRanks(uniqueId: Array[Byte], worldSize: Int, rank: Int): Unit = {
    require(fp64, "a communicator across processes needs -Ddsgd.precision=fp64")
    NativeSVM.commInitF64v(ctx, uniqueId, worldSize, rank)
  }
  def detachRanks(): Unit = NativeSVM.commDestroy(ctx)

  /** body of SlaveImpl.gradient (core/Slave.scala:142-157) */
  def gradientBatch(w: Vec, samplesIdx: Seq[Int]): Vec = {
    val (wk, wv) = SparsePairs.fromVec(w)
    synchronized(take(NativeSVM.gradientSparse(ctx, wk, wv, samplesIdx.toArray, null)))
  }

  /** the pairs a sparse native left in the shim's scratch, as a Vec (called with this object's monitor held) */
  private def take(n: Int): Vec = {
    val keys = new Array[Int](n)
    val vals = new Array[Float](n)
    NativeSVM.takeSparse(ctx, keys, vals)
    SparsePairs.toVec(keys, vals, dim)
  }

  /** body of SlaveImpl.forward (core/Slave.scala:129-140) */
  def forwardBatch(w: Vec, samplesIdx: Seq[Int]): Seq[Number] = {
    val p = new Array[Float](samplesIdx.size)
    NativeSVM.forward(ctx, DenseKeys.fromVec(w), samplesIdx.toArray, p)
    p.map(x => Number(x.toDouble))
  }

  /** Master.localLoss / localAccuracy over a row range (core/Master.scala:100-107).  In resident mode the weights on
    * the device ARE the model's weights and are evaluated IN PLACE (a null `w`: dsgd_loss_acc then writes nothing): the
    * `w` a caller holds is a snapshot of them, and writing it back would discard every update the slave threads applied
    * since it was taken (MasterAsync's loss check runs while they do, core/MasterAsync.scala:96-162). */
  def lossAndAccuracy(w: Vec, rowBegin: Int, rowEnd: Int): (Number, Double) = {
    val out = new Array[Double](2)
    NativeSVM.lossAcc(ctx, if (resident) null else DenseKeys.fromVec(w), rowBegin, rowEnd, out)
    (Number(out(0)), out(1))
  }

  /** Master.predict over the workers' splits (core/Master.scala:61-75) in ONE launch: `ranges` = the splits as [begin, end)
    * row ranges (SplitStrategy.vanilla yields contiguous ones); one Byte in {-1, 0, +1} per row, split after split.  The loss
    * and accuracy the reference folds over the same predictions (:77-98) are kept for lastPredictLoss / lastPredictAccuracy.
    * Resident mode evaluates the weights on the device in place, as lossAndAccuracy does; an fp64 context takes no Float
    * `w` here, so outside resident mode `w` is stored first (setWeights) and then evaluated in place. */
  def predict(w: Vec, ranges: Seq[(Int, Int)]): Array[Byte] = synchronized {
    val p   = new Array[Byte](ranges.map { case (b, e) => math.max(0, e - b) }.sum)
    val out = new Array[Double](2)
    if (fp64 && !resident) setWeights(w)
    NativeSVM.predictRanges(ctx, if (resident || fp64) null else DenseKeys.fromVec(w), ranges.map(_._1.toLong).toArray,
                            ranges.map(_._2.toLong).toArray, p, out)
    predictLoss = out(0)
    predictAccuracy = out(1)
    p
  }
  private var predictLoss: Double     = Double.NaN
  private var predictAccuracy: Double = Double.NaN

  /** Master.distributedLoss / distributedAccuracy (core/Master.scala:77-98) of the last predict call */
  def lastPredictLoss: Number      = synchronized(Number(predictLoss))
  def lastPredictAccuracy: Double = synchronized(predictAccuracy)

  /** Master.localSampledLoss / localSampledAccuracy (core/Master.scala:109-118) over rows [rowBegin, rowEnd): (loss, accuracy,
    * state behind the shuffle).  `state` is the internal 48-bit state of the java.util.Random the reference would shuffle with;
    * the device draws `Random.shuffle(0 until len) take samplesCount` from it and tallies the sample in one launch.  Where the
    * device form does not apply (a window beyond 2^20 rows) UnsupportedOperationException is thrown and nothing was drawn: the
    * caller shuffles on the JVM and calls sampledLossAndAccuracy(w, idx).  The weights as in predict. */
  def sampledLossAndAccuracy(w: Vec, state: Long, rowBegin: Int, rowEnd: Int, samplesCount: Int): (Number, Double, Long) = synchronized {
    val out = new Array[Double](4)
    if (fp64 && !resident) setWeights(w)
    val after = NativeSVM.lossAccSampled(ctx, if (resident || fp64) null else DenseKeys.fromVec(w), state, rowBegin.toLong, rowEnd.toLong,
                                         samplesCount.toLong, out)
    (Number(out(0)), out(1), after)
  }

  /** ... over the rows `idx` names (a sample drawn by the caller; a row named twice counts twice): (loss, accuracy) */
  def sampledLossAndAccuracy(w: Vec, idx: Array[Int]): (Number, Double) = synchronized {
    val out = new Array[Double](2)
    if (fp64 && !resident) setWeights(w)
    NativeSVM.lossAccList(ctx, if (resident || fp64) null else DenseKeys.fromVec(w), idx, out)
    (Number(out(0)), out(1))
  }

  /** dev mode (Main.scala "launch: master + slaves"): master and slaves live in ONE JVM and share this object, i.e. ONE
    * device context holds every row and the weights can stay on the device between batches / iterations. */
  @volatile var resident: Boolean = false

  def setWeights(w: Vec): Unit = {
    val (k, v) = SparsePairs.fromVec(w)
    NativeSVM.setWeightsSparse(ctx, k, v)
  }

  def weights(): Vec = synchronized(take(NativeSVM.getWeightsSparse(ctx)))

  /** the whole batch closure of Master.fit (core/Master.scala:184-197) for the workers hosted by this context: per-worker
    * regularised sums, mean over the workers, w <- w - learningRate * mean.  An empty list fails as Vec.sum does. */
  def syncStep(idxPerWorker: Seq[Seq[Int]], learningRate: Double): Long =
    NativeSVM.syncStep(ctx, idxPerWorker.map(_.toArray).toArray, learningRate.toFloat)

  /** ONE EPOCH of Master.fit's batch loop (core/Master.scala:179-199) for the workers hosted by this context, as one resident
    * plan: `batches(b)(k)` = the sample list of worker k in batch b, i.e. what
    * `split.map(Random.shuffle(_)).slice(batch, batch + batchSize)` (:184) yields, drawn by the caller in the reference's own
    * order.  All batches run in ONE launch of the column-slice kernel (5 us per 3 x 100 batch; `syncStep` per batch costs
    * 40 us plus the JNI array traffic); the weights stay on the device.  Returns the number of active samples of the epoch.
    * An empty list fails as Vec.sum does (math/Vec.scala:129) -- before anything runs. */
  def fitEpoch(batches: Seq[Seq[Seq[Int]]], learningRate: Double): Long = {
    val plan = createEpochPlan(batches)
    try runEpochPlan(plan, batches.size, learningRate)
    finally NativeSVM.planDestroy(ctx, plan)
  }

  /** The two halves of `fitEpoch`, for a master that lays the NEXT epoch's plan out while this epoch's batches run
    * (planCreate works on a stream of its own beside the launch stream). */
  def createEpochPlan(batches: Seq[Seq[Seq[Int]]]): Long = {
    require(batches.nonEmpty, "an epoch needs at least one batch")
    val nWorkers = batches.head.size
    require(batches.forall(_.size == nWorkers), "every batch needs one list per worker")
    val total   = batches.iterator.map(_.iterator.map(_.size).sum).sum
    val idx     = new Array[Int](total)
    val offsets = new Array[Long](batches.size * nWorkers + 1)
    var at, i   = 0
    batches.foreach(_.foreach { list =>
      list.foreach { r => idx(at) = r; at += 1 }
      i += 1
      offsets(i) = at
    })
    try NativeSVM.planCreate(ctx, idx, offsets, nWorkers)
    catch { case e: RuntimeException if refused(e) => NativeSVM.planCreateRp64(ctx, idx, offsets, nWorkers) }
  }

  /** `fitEpoch` with the epoch's sample lists DRAWN BY THE DEVICE -- draw for draw what
    * `split.map(Random.shuffle(_)).slice(batch, batch + batchSize)` (core/Master.scala:184) would have drawn from `rnd`, which is
    * left exactly where those shuffles would have left it.  The reference reshuffles every worker's whole split for EVERY
    * batch: 1.38 G draws per epoch of RCV1 (seconds on the JVM) for 644 K list entries; the device scans the raw stream,
    * the library walks the rejection candidates, and every list is traced backwards through its Fisher-Yates by one
    * workgroup (14 ms).  `split(k)` must be the contiguous range SplitStrategy.vanilla hands worker k.  Returns the number
    * of batches run -- fewer than `0 until maxSamples by batchSize` holds only if a batch would hand some worker an empty
    * slice (the reference's slave throws there: the caller raises the same error) -- or None when the epoch is outside the
    * device form (batches beyond 1,024 rows, splits beyond 2^20 rows): the caller then draws the lists itself (`fitEpoch`). */
  def fitEpochFromSeed(rnd: java.util.Random, split: Seq[Range], maxSamples: Int, batchSize: Int, learningRate: Double): Option[Int] = {
    if (split.exists(r => r.step != 1 || r.isEmpty)) return None
    val seedField = classOf[java.util.Random].getDeclaredField("seed")   // (an AtomicLong; 48 bits, already scrambled)
    seedField.setAccessible(true)
    val seed  = seedField.get(rnd).asInstanceOf[java.util.concurrent.atomic.AtomicLong]
    val state = Array(seed.get(), 0L, 0L)
    val (begins, ends) = (split.map(_.start.toLong).toArray, split.map(r => (r.last + 1).toLong).toArray)
    val plan =
      try NativeSVM.planCreateFromSeed(ctx, state, begins, ends, maxSamples.toLong, batchSize)
      catch {
        case _: UnsupportedOperationException if rpPlans =>   // (state is untouched by a refusal)
          try NativeSVM.planCreateFromSeedRp64(ctx, state, begins, ends, maxSamples.toLong, batchSize)
          catch { case _: UnsupportedOperationException => return None }
        case _: UnsupportedOperationException => return None
      }
    seed.set(state(0))
    if (plan != 0L) {
      try runEpochPlan(plan, state(1).toInt, learningRate)
      finally NativeSVM.planDestroy(ctx, plan)
    }
    Some(state(1).toInt)
  }

  def runEpochPlan(plan: Long, nBatches: Int, learningRate: Double): Long = {
    NativeSVM.planRun(ctx, plan, 0, nBatches, learningRate.toFloat)
    NativeSVM.planSynchronize(ctx)
  }

  def destroyEpochPlan(plan: Long): Unit = NativeSVM.planDestroy(ctx, plan)

  /** one iteration of Slave.asyncTask (core/Slave.scala:92-101) on the device-resident weights; returns the update that
    * is gossiped (core/Slave.scala:103-105) */
  def asyncStepBatch(samplesIdx: Seq[Int], learningRate: Double): Vec =
    synchronized(take(NativeSVM.asyncStepSparse(ctx, samplesIdx.toArray, learningRate.toFloat)))

  /** SlaveImpl.updateGrad / MasterAsync.updateGrad (core/Slave.scala:177-185): w <- w - delta; may arrive while the
    * lock-free engine runs */
  def updateGrad(delta: Vec): Unit = {
    val entries = delta.map.toSeq
    NativeSVM.updateGrad(ctx, entries.map(_._1).toArray, entries.map(_._2.toDouble.toFloat).toArray)
  }

  /** the persistent lock-free engine: `assigned` = one contiguous row range per worker (SplitStrategy.vanilla), all of
    * them updating ONE device-resident weight vector (BASELINE configs[3]); maxUpdates as MasterAsync counts them
    * (core/MasterAsync.scala:83,171) */
  def asyncStart(assigned: Seq[(Int, Int)], batchSize: Int, learningRate: Double, maxUpdates: Long, seed: Long): Unit =
    NativeSVM.asyncStart(ctx, assigned.map(_._1.toLong).toArray, assigned.map(_._2.toLong).toArray, batchSize,
                         learningRate.toFloat, maxUpdates, seed, false)

  def asyncUpdates(): Long = NativeSVM.asyncUpdates(ctx)

  def asyncStop(): Unit = NativeSVM.asyncStop(ctx)

  def asyncWait(): Unit = NativeSVM.asyncWait(ctx)

  def close(): Unit = NativeSVM.destroy(ctx)
}

object HipSVM {
  def isResident(model: SparseSVM): Boolean = model match {
    case h: HipSVM => h.resident
    case _         => false
  }
}
