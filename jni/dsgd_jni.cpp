// JNI shim between the reference's Scala classes and libdsgd_hip (include/dsgd.h).
//
// Build on a box with a JDK:
//   g++ -std=c++17 -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../include
//       dsgd_jni.cpp -o libdsgd_jni.so -L../distributed-sgd_amd/lib -ldsgd_hip        (one command line)
// This image has no JDK; tests/test_jni_shim.py compiles this file against tests/jni_stub/jni.h (a stand-in that
// declares the slice of the JNI API used here), checks the exported symbol set against the @native declarations of
// scala/NativeSVM.scala and drives the entry points with a recording fake JNIEnv.
//
// Symbol names.  The natives are declared in `object NativeSVM` (scala/NativeSVM.scala), i.e. on the JVM class
// `epfl.distributed.core.ml.NativeSVM$`; JNI mangles '$' as `_00024`, and a method of a Scala object is an INSTANCE
// method of the module singleton, so every entry point takes (JNIEnv*, jobject self, ...).
//
// Array passing.  Arrays are taken with Get<Type>ArrayElements / Release<Type>ArrayElements (which may pin or copy
// and put no restriction on what runs in between), never with GetPrimitiveArrayCritical: every dsgd_* call below
// takes the context mutex and blocks on the GPU, which is exactly what a JNI critical region must not do (the
// reference calls its model from an 8-thread pool, utils/Pool.scala:13 -- a thread parked inside a critical region
// stalls every collector).  Array lengths are read before any array is taken.
//
// Error mapping (include/dsgd.h): DSGD_EINVAL -> IllegalArgumentException (what `require` throws at
// math/Vec.scala:129 and math/Sparse.scala:16), DSGD_ERANGE -> IndexOutOfBoundsException
// (math/Sparse.scala:63), everything else -> RuntimeException.
#include <jni.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "dsgd.h"

#define NATIVE(name) Java_epfl_distributed_core_ml_NativeSVM_00024_##name

namespace {
jint raise(JNIEnv* env, int rc) {
  const char* cls = rc == DSGD_EINVAL   ? "java/lang/IllegalArgumentException"
                    : rc == DSGD_ERANGE ? "java/lang/IndexOutOfBoundsException"
                                        : "java/lang/RuntimeException";
  env->ThrowNew(env->FindClass(cls), dsgd_last_error());
  return rc;
}
inline dsgd_ctx* ctx(jlong h) { return reinterpret_cast<dsgd_ctx*>(h); }

// RAII views of primitive arrays.  `mode` 0 copies changes back (outputs), JNI_ABORT discards them (inputs).
// (each view keeps its TYPED array reference: in the JDK's jni.h jlongArray, jintArray, ... are distinct classes derived
// from _jarray, and Get/Release<Type>ArrayElements take exactly their own)
#define DSGD_ELEMS(Name, T, A)                                                                       \
  struct Name##Elems {                                                                               \
    JNIEnv* env;                                                                                     \
    A arr;                                                                                           \
    T* p;                                                                                            \
    jint mode;                                                                                       \
    Name##Elems(JNIEnv* e, A a, jint m)                                                              \
        : env(e), arr(a), p(a ? e->Get##Name##ArrayElements(a, nullptr) : nullptr), mode(m) {}       \
    ~Name##Elems() {                                                                                 \
      if (p) env->Release##Name##ArrayElements(arr, p, mode);                                        \
    }                                                                                                \
    Name##Elems(const Name##Elems&) = delete;                                                        \
    Name##Elems& operator=(const Name##Elems&) = delete;                                             \
  };
DSGD_ELEMS(Long, jlong, jlongArray)
DSGD_ELEMS(Int, jint, jintArray)
DSGD_ELEMS(Float, jfloat, jfloatArray)
DSGD_ELEMS(Byte, jbyte, jbyteArray)
DSGD_ELEMS(Double, jdouble, jdoubleArray)
#undef DSGD_ELEMS

// Sparse values (include/dsgd.h "SPARSE VALUES"): per context, native scratch of D + 1 slots the library compacts into, so
// that the JVM never allocates or scans D + 1 slots.  A sparse native leaves its pairs here and returns their count; the
// caller allocates two arrays of exactly that length and collects them with takeSparse / takeSparseF64 (HipSVM holds its
// monitor across the two calls).
struct SparseScratch {
  std::mutex mu;
  int64_t dp = 0;
  std::vector<int32_t> keys;
  std::vector<double> vals;   // 8-byte slots: floats or doubles
  int64_t nnz = 0;
  bool f64 = false;
};
std::mutex g_scratch_mu;
std::map<jlong, std::shared_ptr<SparseScratch>> g_scratch;
void scratch_add(jlong h, jint nFeatures) {
  auto s = std::make_shared<SparseScratch>();
  s->dp = static_cast<int64_t>(nFeatures) + 1;
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  g_scratch[h] = s;
}
void scratch_drop(jlong h) {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  g_scratch.erase(h);
}
std::shared_ptr<SparseScratch> scratch_of(JNIEnv* env, jlong h) {
  std::shared_ptr<SparseScratch> s;
  {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    auto it = g_scratch.find(h);
    if (it != g_scratch.end()) s = it->second;
  }
  if (!s) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "not a context of this shim (create / createF64)");
    return s;
  }
  if (s->keys.empty()) {
    s->keys.resize(static_cast<size_t>(s->dp));
    s->vals.resize(static_cast<size_t>(s->dp));
  }
  return s;
}
bool null_array(JNIEnv* env) {
  env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "null array");
  return true;
}
bool pair_mismatch(JNIEnv* env, jarray keys, jarray vals) {   // both null (the resident weights) or both of one length
  if ((keys == nullptr) != (vals == nullptr) || (keys && env->GetArrayLength(keys) != env->GetArrayLength(vals))) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "keys / values: both null or of one length");
    return true;
  }
  return false;
}
void set_region(JNIEnv* env, jfloatArray a, jsize n, const jfloat* p) { env->SetFloatArrayRegion(a, 0, n, p); }
void set_region(JNIEnv* env, jdoubleArray a, jsize n, const jdouble* p) { env->SetDoubleArrayRegion(a, 0, n, p); }

// the bodies of the sparse natives, for float and double (the C entry point comes as `fn`); -1 = an exception is pending
template <typename T, typename Elems, typename TArr, typename Fn>
jint gradient_sparse(JNIEnv* env, jlong h, jintArray wKeys, TArr wVals, jintArray idx, jlongArray statsOut, bool is64, Fn fn) {
  if (!idx && null_array(env)) return -1;
  if (pair_mismatch(env, wKeys, wVals)) return -1;
  auto s = scratch_of(env, h);
  if (!s) return -1;
  const jsize n = env->GetArrayLength(idx);
  const int64_t wn = wKeys ? env->GetArrayLength(wKeys) : -1;
  dsgd_batch_stats st{};
  std::lock_guard<std::mutex> lk(s->mu);
  int rc;
  {
    IntElems kv(env, wKeys, JNI_ABORT);
    Elems vv(env, wVals, JNI_ABORT);
    IntElems iv(env, idx, JNI_ABORT);
    rc = fn(ctx(h), reinterpret_cast<const int32_t*>(kv.p), vv.p, wn, reinterpret_cast<const int32_t*>(iv.p), n, s->keys.data(),
            reinterpret_cast<T*>(s->vals.data()), s->dp, &s->nnz, &st);
  }
  if (rc) {
    s->nnz = 0;
    raise(env, rc);
    return -1;
  }
  s->f64 = is64;
  if (statsOut && env->GetArrayLength(statsOut) >= 1) {
    const jlong a = st.n_active;
    env->SetLongArrayRegion(statsOut, 0, 1, &a);
  }
  return static_cast<jint>(s->nnz);
}
template <typename T, typename Lr, typename Fn>
jint async_step_sparse(JNIEnv* env, jlong h, jintArray idx, Lr lr, bool is64, Fn fn) {
  if (!idx && null_array(env)) return -1;
  auto s = scratch_of(env, h);
  if (!s) return -1;
  const jsize n = env->GetArrayLength(idx);
  std::lock_guard<std::mutex> lk(s->mu);
  int rc;
  {
    IntElems iv(env, idx, JNI_ABORT);
    rc = fn(ctx(h), reinterpret_cast<const int32_t*>(iv.p), n, lr, s->keys.data(), reinterpret_cast<T*>(s->vals.data()), s->dp, &s->nnz,
            nullptr);
  }
  if (rc) {
    s->nnz = 0;
    raise(env, rc);
    return -1;
  }
  s->f64 = is64;
  return static_cast<jint>(s->nnz);
}
template <typename T, typename Fn>
jint get_weights_sparse(JNIEnv* env, jlong h, bool is64, Fn fn) {
  auto s = scratch_of(env, h);
  if (!s) return -1;
  std::lock_guard<std::mutex> lk(s->mu);
  const int rc = fn(ctx(h), s->keys.data(), reinterpret_cast<T*>(s->vals.data()), s->dp, &s->nnz);
  if (rc) {
    s->nnz = 0;
    raise(env, rc);
    return -1;
  }
  s->f64 = is64;
  return static_cast<jint>(s->nnz);
}
template <typename Elems, typename TArr, typename Fn>
void set_weights_sparse(JNIEnv* env, jlong h, jintArray keys, TArr vals, Fn fn) {
  if ((!keys || !vals) && null_array(env)) return;
  if (pair_mismatch(env, keys, vals)) return;
  const jsize n = env->GetArrayLength(keys);
  int rc;
  {
    IntElems kv(env, keys, JNI_ABORT);
    Elems vv(env, vals, JNI_ABORT);
    rc = fn(ctx(h), reinterpret_cast<const int32_t*>(kv.p), vv.p, n);
  }
  if (rc) raise(env, rc);
}
template <typename T, typename TArr>
void take_sparse(JNIEnv* env, jlong h, jintArray keysOut, TArr valsOut, bool is64) {
  if ((!keysOut || !valsOut) && null_array(env)) return;
  auto s = scratch_of(env, h);
  if (!s) return;
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->f64 != is64 || env->GetArrayLength(keysOut) != s->nnz || env->GetArrayLength(valsOut) != s->nnz) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "the arrays do not match the pairs held for this context");
    return;
  }
  env->SetIntArrayRegion(keysOut, 0, static_cast<jsize>(s->nnz), reinterpret_cast<const jint*>(s->keys.data()));
  set_region(env, valsOut, static_cast<jsize>(s->nnz), reinterpret_cast<const T*>(s->vals.data()));
}
}  // namespace

extern "C" {

// new SparseSVM(lambda, dimSparsity) + the data array given to `new Slave(...)` (Main.scala:68,138,148)
JNIEXPORT jlong JNICALL NATIVE(create)(JNIEnv* env, jobject, jint nFeatures, jdouble lambda, jint device) {
  dsgd_config cfg{};
  cfg.n_features = nFeatures;
  cfg.device = device;
  cfg.lambda = lambda;
  dsgd_ctx* c = nullptr;
  int rc = dsgd_create(&cfg, &c);
  if (rc) {
    raise(env, rc);
    return 0;
  }
  scratch_add(reinterpret_cast<jlong>(c), nFeatures);
  return reinterpret_cast<jlong>(c);
}

JNIEXPORT void JNICALL NATIVE(destroy)(JNIEnv*, jobject, jlong h) {
  scratch_drop(h);
  dsgd_destroy(ctx(h));
}

// the same in the fp64 mode (DSGD_F_FP64, include/dsgd.h "THE FP64 MODE"): the reference's Double weights and learning rate
JNIEXPORT jlong JNICALL NATIVE(createF64)(JNIEnv* env, jobject, jint nFeatures, jdouble lambda, jint device) {
  dsgd_config cfg{};
  cfg.n_features = nFeatures;
  cfg.device = device;
  cfg.lambda = lambda;
  cfg.flags = DSGD_F_FP64;
  dsgd_ctx* c = nullptr;
  int rc = dsgd_create(&cfg, &c);
  if (rc) {
    raise(env, rc);
    return 0;
  }
  scratch_add(reinterpret_cast<jlong>(c), nFeatures);
  return reinterpret_cast<jlong>(c);
}

JNIEXPORT void JNICALL NATIVE(setWeightsF64)(JNIEnv* env, jobject, jlong h, jdoubleArray w) {
  int rc;
  {
    DoubleElems wv(env, w, JNI_ABORT);
    rc = dsgd_set_weights_f64(ctx(h), wv.p);
  }
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(getWeightsF64)(JNIEnv* env, jobject, jlong h, jdoubleArray wOut) {
  int rc;
  {
    DoubleElems wv(env, wOut, 0);
    rc = dsgd_get_weights_f64(ctx(h), wv.p);
  }
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(planRunF64)(JNIEnv* env, jobject, jlong h, jlong plan, jlong stepBegin, jlong stepEnd, jdouble lr) {
  int rc = dsgd_plan_run_f64(ctx(h), reinterpret_cast<dsgd_plan*>(plan), stepBegin, stepEnd, lr);
  if (rc) raise(env, rc);
}

// Array[(Vec, Int)] flattened by the Scala side to CSR (utils/Dataset.scala:11)
JNIEXPORT void JNICALL NATIVE(loadCsr)(JNIEnv* env, jobject, jlong h, jlongArray rowPtr, jintArray col, jfloatArray val,
                                       jbyteArray label) {
  const jsize nRows = env->GetArrayLength(label);
  int rc;
  {
    LongElems rp(env, rowPtr, JNI_ABORT);
    IntElems c(env, col, JNI_ABORT);
    FloatElems v(env, val, JNI_ABORT);
    ByteElems y(env, label, JNI_ABORT);
    rc = dsgd_load_csr(ctx(h), nRows, reinterpret_cast<const int64_t*>(rp.p), reinterpret_cast<const int32_t*>(c.p), v.p,
                       reinterpret_cast<const int8_t*>(y.p));
  }
  if (rc) raise(env, rc);
}

// the same rows with the Vec's Double values as they are (an fp64 context: include/dsgd.h "THE FP64 MODE", Double feature values)
JNIEXPORT void JNICALL NATIVE(loadCsrF64)(JNIEnv* env, jobject, jlong h, jlongArray rowPtr, jintArray col, jdoubleArray val,
                                          jbyteArray label) {
  if (!rowPtr || !col || !val || !label || env->GetArrayLength(col) != env->GetArrayLength(val) ||
      env->GetArrayLength(rowPtr) != env->GetArrayLength(label) + 1) {   // (refused before any array is taken)
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "null array, or rowPtr / col / value / label lengths that do not fit");
    return;
  }
  const jsize nRows = env->GetArrayLength(label);
  int rc;
  {
    LongElems rp(env, rowPtr, JNI_ABORT);
    IntElems c(env, col, JNI_ABORT);
    DoubleElems v(env, val, JNI_ABORT);
    ByteElems y(env, label, JNI_ABORT);
    rc = dsgd_load_csr_f64(ctx(h), nRows, reinterpret_cast<const int64_t*>(rp.p), reinterpret_cast<const int32_t*>(c.p), v.p,
                           reinterpret_cast<const int8_t*>(y.p));
  }
  if (rc) raise(env, rc);
}

// Main.scala:54-65 on the device
JNIEXPORT void JNICALL NATIVE(buildDimSparsity)(JNIEnv* env, jobject, jlong h, jlong nTrain) {
  int rc = dsgd_build_dim_sparsity(ctx(h), nTrain, nullptr);
  if (rc) raise(env, rc);
}

// SlaveImpl.gradient (core/Slave.scala:142-157); w may be null = use the resident weights.
// Returns the number of active samples so that the caller can counter.increment(n) (Slave.scala:145,150).
JNIEXPORT jlong JNICALL NATIVE(gradient)(JNIEnv* env, jobject, jlong h, jfloatArray w, jintArray idx, jfloatArray gOut) {
  dsgd_batch_stats st{};
  const jsize n = env->GetArrayLength(idx);
  int rc;
  {
    FloatElems wv(env, w, JNI_ABORT);
    IntElems iv(env, idx, JNI_ABORT);
    FloatElems gv(env, gOut, 0);
    rc = dsgd_gradient(ctx(h), wv.p, reinterpret_cast<const int32_t*>(iv.p), n, gv.p, &st);
  }
  if (rc) raise(env, rc);
  return st.n_active;
}

// SlaveImpl.forward (core/Slave.scala:129-140)
JNIEXPORT void JNICALL NATIVE(forward)(JNIEnv* env, jobject, jlong h, jfloatArray w, jintArray idx, jfloatArray predOut) {
  const jsize n = env->GetArrayLength(idx);
  int rc;
  {
    FloatElems wv(env, w, JNI_ABORT);
    IntElems iv(env, idx, JNI_ABORT);
    FloatElems pv(env, predOut, 0);
    rc = dsgd_forward(ctx(h), wv.p, reinterpret_cast<const int32_t*>(iv.p), n, pv.p);
  }
  if (rc) raise(env, rc);
}

// Master.fit batch closure (core/Master.scala:184-197) for the workers hosted by this process
JNIEXPORT jlong JNICALL NATIVE(syncStep)(JNIEnv* env, jobject, jlong h, jobjectArray idxPerWorker, jfloat lr) {
  const jsize k = env->GetArrayLength(idxPerWorker);
  // index lists are small (batch-size entries): copied out with GetIntArrayRegion
  std::vector<std::vector<int32_t>> lists(static_cast<size_t>(k));
  std::vector<const int32_t*> ptrs(static_cast<size_t>(k));
  std::vector<int64_t> ns(static_cast<size_t>(k));
  for (jsize i = 0; i < k; ++i) {
    jintArray a = static_cast<jintArray>(env->GetObjectArrayElement(idxPerWorker, i));
    const jsize n = a ? env->GetArrayLength(a) : 0;
    lists[i].resize(n > 0 ? n : 1);
    if (n > 0) env->GetIntArrayRegion(a, 0, n, reinterpret_cast<jint*>(lists[i].data()));
    ptrs[i] = lists[i].data();
    ns[i] = n;
    if (a) env->DeleteLocalRef(a);
  }
  dsgd_batch_stats st{};
  int rc = dsgd_sync_step(ctx(h), ptrs.data(), ns.data(), k, lr, &st);
  if (rc) raise(env, rc);
  return st.n_active;
}

// ---- an EPOCH of Master.fit as ONE resident plan (core/Master.scala:179-199) ---------------------------------------
// The epoch loop draws `split.map(Random.shuffle(_)).slice(batch, batch + batchSize)` for every batch (:184) -- nothing else
// consumes the generator inside the loop -- so the patched Master.fit draws the epoch's lists first, in the reference's
// own order, and hands them over flattened: idx = all lists concatenated (batch-major, worker-minor), offsets = nSteps *
// nWorkers + 1 prefix offsets.  planRun(0, nSteps) then runs the whole epoch in ONE launch of the column-slice kernel
// (5 us per 3 x 100 batch against 40 us per syncStep call); planCreate lays the lists out on the device beside whatever is
// running, so the next epoch's plan can be created while this epoch's batches run.
static jlong plan_create(JNIEnv* env, jlong h, jintArray idx, jlongArray offsets, jint nWorkers, bool rp64) {
  const jsize nOff = env->GetArrayLength(offsets);
  if (nWorkers < 1 || nOff < 1 || (nOff - 1) % nWorkers != 0) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "offsets must hold nSteps * nWorkers + 1 entries");
    return 0;
  }
  dsgd_plan* plan = nullptr;
  int rc;
  {
    IntElems iv(env, idx, JNI_ABORT);
    LongElems ov(env, offsets, JNI_ABORT);
    // (the stated length: offsets that end beyond the pinned array are refused instead of read)
    rc = (rp64 ? dsgd_plan_create_rp64_n : dsgd_plan_create_n)(ctx(h), reinterpret_cast<const int32_t*>(iv.p), (int64_t)env->GetArrayLength(idx),
                                                               reinterpret_cast<const int64_t*>(ov.p), (nOff - 1) / nWorkers, nWorkers, &plan);
  }
  if (rc) {
    raise(env, rc);
    return 0;
  }
  return reinterpret_cast<jlong>(plan);
}
JNIEXPORT jlong JNICALL NATIVE(planCreate)(JNIEnv* env, jobject, jlong h, jintArray idx, jlongArray offsets, jint nWorkers) {
  return plan_create(env, h, idx, offsets, nWorkers, false);
}
// The same lists as a ROW-PARALLEL plan of an fp64 context (dsgd_plan_create_rp64_n; include/dsgd.h "THE FP64 MODE", ROW-PARALLEL
// PLANS): what planCreate refuses there -- Double feature values, more than 4 workers, more than 1,024 rows per batch, a model
// beyond a slice's LDS.  planRun / planRunF64 / planSynchronize / planDestroy serve it like any plan.
JNIEXPORT jlong JNICALL NATIVE(planCreateRp64)(JNIEnv* env, jobject, jlong h, jintArray idx, jlongArray offsets, jint nWorkers) {
  return plan_create(env, h, idx, offsets, nWorkers, true);
}

// The same epoch with its lists DRAWN BY THE DEVICE, draw for draw scala.util.Random's stream (dsgd_plan_create_from_seed:
// core/Master.scala:184 costs 1.38 G draws per epoch of RCV1 -- seconds on the JVM, 14 ms here).  state = {java.util.Random's
// internal 48-bit seed in front of the epoch (HipSVM reads and writes it by reflection), out: batches emitted, out: raw
// values consumed}; on return state[0] is where the JVM's generator would stand behind the epoch's last shuffle.  Returns 0
// with state[1] = 0 when the first batch already hands a worker an empty slice.  An epoch outside the device form's limits
// raises UnsupportedOperationException: the caller draws the lists itself and uses planCreate.
static jlong plan_create_from_seed(JNIEnv* env, jlong h, jlongArray state, jlongArray splitBegin, jlongArray splitEnd, jlong maxSamples,
                                   jint batchSize, bool rp64) {
  const jsize n = env->GetArrayLength(splitBegin);
  if (env->GetArrayLength(state) < 3 || n < 1 || env->GetArrayLength(splitEnd) != n) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "state must hold 3 entries, splitBegin / splitEnd one per worker");
    return 0;
  }
  dsgd_plan* plan = nullptr;
  int rc;
  {
    LongElems sv(env, state, 0);
    LongElems bv(env, splitBegin, JNI_ABORT);
    LongElems ev(env, splitEnd, JNI_ABORT);
    uint64_t js = (uint64_t)sv.p[0];
    int64_t n_steps = 0, draws = 0;
    rc = (rp64 ? dsgd_plan_create_from_seed_rp64 : dsgd_plan_create_from_seed)(ctx(h), &js, reinterpret_cast<const int64_t*>(bv.p),
                                                                               reinterpret_cast<const int64_t*>(ev.p), (int32_t)n, (int64_t)maxSamples,
                                                                               (int32_t)batchSize, &plan, &n_steps, &draws);
    if (rc == DSGD_OK) {
      sv.p[0] = (jlong)js;
      sv.p[1] = (jlong)n_steps;
      sv.p[2] = (jlong)draws;
    }
  }
  if (rc == DSGD_EUNSUPPORTED) {
    env->ThrowNew(env->FindClass("java/lang/UnsupportedOperationException"), dsgd_last_error());
    return 0;
  }
  if (rc) {
    raise(env, rc);
    return 0;
  }
  return reinterpret_cast<jlong>(plan);
}
JNIEXPORT jlong JNICALL NATIVE(planCreateFromSeed)(JNIEnv* env, jobject, jlong h, jlongArray state, jlongArray splitBegin,
                                                   jlongArray splitEnd, jlong maxSamples, jint batchSize) {
  return plan_create_from_seed(env, h, state, splitBegin, splitEnd, maxSamples, batchSize, false);
}
// ... into a row-parallel plan of an fp64 context (dsgd_plan_create_from_seed_rp64): the same draws, the same state behind them
JNIEXPORT jlong JNICALL NATIVE(planCreateFromSeedRp64)(JNIEnv* env, jobject, jlong h, jlongArray state, jlongArray splitBegin,
                                                       jlongArray splitEnd, jlong maxSamples, jint batchSize) {
  return plan_create_from_seed(env, h, state, splitBegin, splitEnd, maxSamples, batchSize, true);
}
// The same epoch for a JOB's share of workers (dsgd_plan_create_from_seed_job / _rp64; include/dsgd.h): jobLen = the split length
// of EVERY worker of the job in the master's order, this context hosts job workers first .. first + splitBegin.length - 1 over
// the rows [splitBegin[i], splitBegin[i] + jobLen[first + i]) it has loaded.  Any batch size; a local call that a communicator does
// not refuse.  state as planCreateFromSeed takes and leaves it -- the JOB's state and draws, the same on every rank.
JNIEXPORT jlong JNICALL NATIVE(planCreateFromSeedJob)(JNIEnv* env, jobject, jlong h, jlongArray state, jlongArray jobLen, jint first,
                                                      jlongArray splitBegin, jlong maxSamples, jint batchSize, jboolean rp64) {
  if (!state || !jobLen || !splitBegin) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "state, jobLen and splitBegin must not be null");
    return 0;
  }
  const jsize nJob = env->GetArrayLength(jobLen), nLocal = env->GetArrayLength(splitBegin);
  if (env->GetArrayLength(state) < 3 || nJob < 1 || nLocal < 1 || first < 0 || (int64_t)first + nLocal > (int64_t)nJob) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"),
                  "state must hold 3 entries, jobLen one per worker of the job, splitBegin one per hosted worker first .. of them");
    return 0;
  }
  dsgd_plan* plan = nullptr;
  int rc;
  {
    LongElems sv(env, state, 0);
    LongElems lv(env, jobLen, JNI_ABORT);
    LongElems bv(env, splitBegin, JNI_ABORT);
    uint64_t js = (uint64_t)sv.p[0];
    int64_t n_steps = 0, draws = 0;
    rc = (rp64 ? dsgd_plan_create_from_seed_job_rp64 : dsgd_plan_create_from_seed_job)(
        ctx(h), &js, reinterpret_cast<const int64_t*>(lv.p), (int32_t)nJob, (int32_t)first, (int32_t)nLocal,
        reinterpret_cast<const int64_t*>(bv.p), (int64_t)maxSamples, (int32_t)batchSize, &plan, &n_steps, &draws);
    if (rc == DSGD_OK) {
      sv.p[0] = (jlong)js;
      sv.p[1] = (jlong)n_steps;
      sv.p[2] = (jlong)draws;
    }
  }
  if (rc == DSGD_EUNSUPPORTED) {
    env->ThrowNew(env->FindClass("java/lang/UnsupportedOperationException"), dsgd_last_error());
    return 0;
  }
  if (rc) {
    raise(env, rc);
    return 0;
  }
  return reinterpret_cast<jlong>(plan);
}
// Updates [firstUpdate, firstUpdate + nUpdates) of the fp64 mode's zero-lag asynchronous schedule as a one-worker row-parallel
// plan whose lists the device draws (dsgd_async_plan_create_rp64): the lock-free engine's sampler for the workers' row ranges,
// batch, seed and positionalBug as asyncStart takes them; Double or float feature values, any batch, any model width.
JNIEXPORT jlong JNICALL NATIVE(asyncPlanCreateRp64)(JNIEnv* env, jobject, jlong h, jlongArray assignedBegin, jlongArray assignedEnd, jint batch,
                                                    jlong seed, jboolean positionalBug, jlong firstUpdate, jlong nUpdates) {
  const jsize n = env->GetArrayLength(assignedBegin);
  if (n < 1 || env->GetArrayLength(assignedEnd) != n) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "assignedBegin / assignedEnd hold one entry per worker");
    return 0;
  }
  dsgd_plan* plan = nullptr;
  int rc;
  {
    LongElems bv(env, assignedBegin, JNI_ABORT);
    LongElems ev(env, assignedEnd, JNI_ABORT);
    rc = dsgd_async_plan_create_rp64(ctx(h), reinterpret_cast<const int64_t*>(bv.p), reinterpret_cast<const int64_t*>(ev.p), (int32_t)n,
                                     (int32_t)batch, (uint64_t)seed, positionalBug ? 1 : 0, (int64_t)firstUpdate, (int64_t)nUpdates, &plan);
  }
  if (rc) {
    raise(env, rc);
    return 0;
  }
  return reinterpret_cast<jlong>(plan);
}

// the batches [stepBegin, stepEnd) of the plan; enqueued -- planSynchronize (or anything that reads the weights) waits
JNIEXPORT void JNICALL NATIVE(planRun)(JNIEnv* env, jobject, jlong h, jlong plan, jlong stepBegin, jlong stepEnd, jfloat lr) {
  int rc = dsgd_plan_run(ctx(h), reinterpret_cast<dsgd_plan*>(plan), stepBegin, stepEnd, lr);
  if (rc) raise(env, rc);
}

// waits for the batches enqueued so far; returns the number of ACTIVE samples among them (errors of the run surface here)
JNIEXPORT jlong JNICALL NATIVE(planSynchronize)(JNIEnv* env, jobject, jlong h) {
  dsgd_batch_stats st{};
  int rc = dsgd_synchronize(ctx(h), &st);
  if (rc) raise(env, rc);
  return st.n_active;
}

JNIEXPORT void JNICALL NATIVE(planDestroy)(JNIEnv* env, jobject, jlong h, jlong plan) {
  int rc = dsgd_plan_destroy(ctx(h), reinterpret_cast<dsgd_plan*>(plan));
  if (rc) raise(env, rc);
}

// the same closure when every worker's batch is its whole split (batch-size >= split size): contiguous row ranges
JNIEXPORT jlong JNICALL NATIVE(syncStepRanges)(JNIEnv* env, jobject, jlong h, jlongArray rowBegin, jlongArray rowEnd,
                                              jfloat lr) {
  const jsize k = env->GetArrayLength(rowBegin);
  if (env->GetArrayLength(rowEnd) != k) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "rowBegin / rowEnd length mismatch");
    return 0;
  }
  dsgd_batch_stats st{};
  int rc;
  {
    LongElems rb(env, rowBegin, JNI_ABORT);
    LongElems re(env, rowEnd, JNI_ABORT);
    rc = dsgd_sync_step_ranges(ctx(h), reinterpret_cast<const int64_t*>(rb.p), reinterpret_cast<const int64_t*>(re.p), k,
                               lr, &st);
  }
  if (rc) raise(env, rc);
  return st.n_active;
}

// Master.localLoss / localAccuracy (core/Master.scala:100-107): out = {loss, accuracy}
JNIEXPORT void JNICALL NATIVE(lossAcc)(JNIEnv* env, jobject, jlong h, jfloatArray w, jlong rowBegin, jlong rowEnd,
                                       jdoubleArray out) {
  double la[2] = {0, 0};
  int rc;
  {
    FloatElems wv(env, w, JNI_ABORT);
    rc = dsgd_loss_acc(ctx(h), wv.p, rowBegin, rowEnd, &la[0], &la[1], nullptr);
  }
  if (rc) {
    raise(env, rc);
    return;
  }
  env->SetDoubleArrayRegion(out, 0, 2, la);
}

// Master.predict / distributedLoss / distributedAccuracy (core/Master.scala:61-98) for the workers hosted by this context:
// range k = worker k's split; predOut gets one byte in {-1, 0, +1} per row, range-major; out = {loss, accuracy}.
// w may be null (the resident weights; the only form an fp64 context takes).  The ranges are a few words: copied out
// first, so that predOut's length is checked against their rows before any array is taken.
JNIEXPORT void JNICALL NATIVE(predictRanges)(JNIEnv* env, jobject, jlong h, jfloatArray w, jlongArray rowBegin, jlongArray rowEnd,
                                             jbyteArray predOut, jdoubleArray out) {
  if ((!rowBegin || !rowEnd || !predOut || !out) && null_array(env)) return;
  const jsize k = env->GetArrayLength(rowBegin);
  if (env->GetArrayLength(rowEnd) != k || env->GetArrayLength(out) < 2) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "rowBegin / rowEnd length mismatch, or out shorter than 2");
    return;
  }
  std::vector<jlong> rb(static_cast<size_t>(k > 0 ? k : 1)), re(static_cast<size_t>(k > 0 ? k : 1));
  if (k > 0) {
    env->GetLongArrayRegion(rowBegin, 0, k, rb.data());
    env->GetLongArrayRegion(rowEnd, 0, k, re.data());
  }
  // (ranges the library refuses -- begin > end, rows outside the data -- write nothing; the others' rows are counted here)
  const jlong room = env->GetArrayLength(predOut);
  jlong total = 0;
  for (jsize i = 0; i < k && total <= room; ++i)
    if (rb[i] >= 0 && re[i] > rb[i]) total = re[i] - rb[i] > room - total ? room + 1 : total + (re[i] - rb[i]);
  if (total > room) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "predOut is shorter than the ranges' rows");
    return;
  }
  double la[2] = {0, 0};
  int rc;
  {
    FloatElems wv(env, w, JNI_ABORT);
    ByteElems pv(env, predOut, 0);
    rc = dsgd_predict_ranges(ctx(h), wv.p, reinterpret_cast<const int64_t*>(rb.data()), reinterpret_cast<const int64_t*>(re.data()), k,
                             reinterpret_cast<int8_t*>(pv.p), nullptr, &la[0], &la[1]);
  }
  if (rc) {
    raise(env, rc);
    return;
  }
  env->SetDoubleArrayRegion(out, 0, 2, la);
}

// Master.localSampledLoss / localSampledAccuracy (core/Master.scala:109-118) over a list drawn by the caller
// (dsgd_loss_acc_list): out = {loss, accuracy}.  w may be null (the resident weights; the only form an fp64 context takes).
JNIEXPORT void JNICALL NATIVE(lossAccList)(JNIEnv* env, jobject, jlong h, jfloatArray w, jintArray idx, jdoubleArray out) {
  if ((!idx || !out) && null_array(env)) return;
  if (env->GetArrayLength(out) < 2) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "out shorter than 2");
    return;
  }
  const jsize n = env->GetArrayLength(idx);
  double la[2] = {0, 0};
  int rc;
  {
    FloatElems wv(env, w, JNI_ABORT);
    IntElems iv(env, idx, JNI_ABORT);
    rc = dsgd_loss_acc_list(ctx(h), wv.p, reinterpret_cast<const int32_t*>(iv.p), n, &la[0], &la[1], nullptr);
  }
  if (rc) {
    raise(env, rc);
    return;
  }
  env->SetDoubleArrayRegion(out, 0, 2, la);
}
// ... over a sample the DEVICE draws (dsgd_loss_acc_sampled): state = java.util.Random's internal 48-bit state in front of the
// shuffle, the return value the state behind it (planCreateFromSeed's meaning of the word, here by value); out = {loss,
// accuracy, rows evaluated, raw values drawn}.  Beyond the device form's limits UnsupportedOperationException is thrown and
// nothing was drawn: shuffle on the JVM and call lossAccList.
JNIEXPORT jlong JNICALL NATIVE(lossAccSampled)(JNIEnv* env, jobject, jlong h, jfloatArray w, jlong state, jlong rowBegin, jlong rowEnd,
                                               jlong samplesCount, jdoubleArray out) {
  if (!out && null_array(env)) return state;
  if (env->GetArrayLength(out) < 4) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "out shorter than 4");
    return state;
  }
  double la[4] = {0, 0, 0, 0};
  uint64_t js = (uint64_t)state;
  int64_t n = 0, draws = 0;
  int rc;
  {
    FloatElems wv(env, w, JNI_ABORT);
    rc = dsgd_loss_acc_sampled(ctx(h), wv.p, &js, rowBegin, rowEnd, samplesCount, &la[0], &la[1], nullptr, nullptr, &n, &draws);
  }
  if (rc == DSGD_EUNSUPPORTED) {
    env->ThrowNew(env->FindClass("java/lang/UnsupportedOperationException"), dsgd_last_error());
    return state;
  }
  if (rc) {
    raise(env, rc);
    return state;
  }
  la[2] = (double)n;
  la[3] = (double)draws;
  env->SetDoubleArrayRegion(out, 0, 4, la);
  return (jlong)js;
}

// Slave.asyncTask body (core/Slave.scala:92-101); deltaOut receives what Slave.scala:103-105 gossips
JNIEXPORT void JNICALL NATIVE(asyncStep)(JNIEnv* env, jobject, jlong h, jintArray idx, jfloat lr, jfloatArray deltaOut) {
  const jsize n = env->GetArrayLength(idx);
  int rc;
  {
    IntElems iv(env, idx, JNI_ABORT);
    FloatElems dv(env, deltaOut, 0);
    rc = dsgd_async_step(ctx(h), reinterpret_cast<const int32_t*>(iv.p), n, lr, dv.p, nullptr);
  }
  if (rc) raise(env, rc);
}

// SlaveImpl.updateGrad / MasterAsync.updateGrad (core/Slave.scala:177-185, core/MasterAsync.scala:164-177)
JNIEXPORT void JNICALL NATIVE(updateGrad)(JNIEnv* env, jobject, jlong h, jintArray keys, jfloatArray values) {
  const jsize n = env->GetArrayLength(keys);
  if (env->GetArrayLength(values) != n) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "keys / values length mismatch");
    return;
  }
  int rc;
  {
    IntElems kv(env, keys, JNI_ABORT);
    FloatElems vv(env, values, JNI_ABORT);
    rc = dsgd_update_grad(ctx(h), reinterpret_cast<const int32_t*>(kv.p), vv.p, n);
  }
  if (rc) raise(env, rc);
}

// the same two in the fp64 mode (include/dsgd.h "THE FP64 MODE"): Double learning rate, delta and values.  Null arrays
// are refused before any array is taken; deltaOut holds D+1 doubles (key order), as the float form's D+1 floats.
JNIEXPORT void JNICALL NATIVE(asyncStepF64)(JNIEnv* env, jobject, jlong h, jintArray idx, jdouble lr, jdoubleArray deltaOut) {
  if (!idx || !deltaOut) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "null array");
    return;
  }
  const jsize n = env->GetArrayLength(idx);
  int rc;
  {
    IntElems iv(env, idx, JNI_ABORT);
    DoubleElems dv(env, deltaOut, 0);
    rc = dsgd_async_step_f64(ctx(h), reinterpret_cast<const int32_t*>(iv.p), n, lr, dv.p, nullptr);
  }
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(updateGradF64)(JNIEnv* env, jobject, jlong h, jintArray keys, jdoubleArray values) {
  if (!keys || !values) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "null array");
    return;
  }
  const jsize n = env->GetArrayLength(keys);
  if (env->GetArrayLength(values) != n) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "keys / values length mismatch");
    return;
  }
  int rc;
  {
    IntElems kv(env, keys, JNI_ABORT);
    DoubleElems vv(env, values, JNI_ABORT);
    rc = dsgd_update_grad_f64(ctx(h), reinterpret_cast<const int32_t*>(kv.p), vv.p, n);
  }
  if (rc) raise(env, rc);
}

// SlaveImpl.gradient / forward in the fp64 mode (dsgd_gradient_f64 / dsgd_forward_f64): the request's Double weights
// (w may be null = the resident fp64 weights), any number of samples.  Null idx / output arrays are refused before any
// array is taken; gOut holds D+1 doubles (key order), predOut one double per sample.
JNIEXPORT jlong JNICALL NATIVE(gradientF64)(JNIEnv* env, jobject, jlong h, jdoubleArray w, jintArray idx, jdoubleArray gOut) {
  if (!idx || !gOut) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "null array");
    return 0;
  }
  dsgd_batch_stats st{};
  const jsize n = env->GetArrayLength(idx);
  int rc;
  {
    DoubleElems wv(env, w, JNI_ABORT);
    IntElems iv(env, idx, JNI_ABORT);
    DoubleElems gv(env, gOut, 0);
    rc = dsgd_gradient_f64(ctx(h), wv.p, reinterpret_cast<const int32_t*>(iv.p), n, gv.p, &st);
  }
  if (rc) raise(env, rc);
  return st.n_active;
}

JNIEXPORT void JNICALL NATIVE(forwardF64)(JNIEnv* env, jobject, jlong h, jdoubleArray w, jintArray idx, jdoubleArray predOut) {
  if (!idx || !predOut) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "null array");
    return;
  }
  const jsize n = env->GetArrayLength(idx);
  if (env->GetArrayLength(predOut) != n) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "idx / predOut length mismatch");
    return;
  }
  int rc;
  {
    DoubleElems wv(env, w, JNI_ABORT);
    IntElems iv(env, idx, JNI_ABORT);
    DoubleElems pv(env, predOut, 0);
    rc = dsgd_forward_f64(ctx(h), wv.p, reinterpret_cast<const int32_t*>(iv.p), n, pv.p);
  }
  if (rc) raise(env, rc);
}

// An epoch's steps of the fp64 mode in ONE call (dsgd_sync_steps_f64): what planCreate + planRunF64 do where the plans
// apply, for everything they refuse (more than 4 workers, more than 1,024 rows per step, Double feature values) -- the
// lists in planCreate's flat form, the bits of one dsgd_sync_step_f64 per step.  activeOut (may be null): nSteps longs,
// each step's active rows.  Returns the active rows of all steps.  Under a communicator: UnsupportedOperationException.
JNIEXPORT jlong JNICALL NATIVE(syncStepsF64)(JNIEnv* env, jobject, jlong h, jintArray idx, jlongArray offsets, jint nWorkers, jdouble lr,
                                             jlongArray activeOut) {
  if (!idx || !offsets) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "null array");
    return 0;
  }
  const jsize nOff = env->GetArrayLength(offsets);
  if (nWorkers < 1 || nOff < 1 || (nOff - 1) % nWorkers != 0) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "offsets must hold nSteps * nWorkers + 1 entries");
    return 0;
  }
  const jsize nSteps = (nOff - 1) / nWorkers;
  if (activeOut && env->GetArrayLength(activeOut) != nSteps) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "activeOut must hold one entry per step");
    return 0;
  }
  dsgd_batch_stats st{};
  int rc;
  {
    IntElems iv(env, idx, JNI_ABORT);
    LongElems ov(env, offsets, JNI_ABORT);
    LongElems av(env, activeOut, 0);
    rc = dsgd_sync_steps_f64(ctx(h), reinterpret_cast<const int32_t*>(iv.p), (int64_t)env->GetArrayLength(idx),
                             reinterpret_cast<const int64_t*>(ov.p), nSteps, nWorkers, lr, reinterpret_cast<int64_t*>(av.p), &st);
  }
  if (rc) raise(env, rc);
  return st.n_active;
}

// ---- Sparse values (include/dsgd.h "SPARSE VALUES"): Vec maps in and out as (keys, values) pairs -----------------------
// A producing native compacts into the context's scratch and returns the count (-1 with an exception pending); takeSparse /
// takeSparseF64 copy the pairs into arrays of exactly that length.  Null arrays are refused before any array is taken.
JNIEXPORT jint JNICALL NATIVE(gradientSparse)(JNIEnv* env, jobject, jlong h, jintArray wKeys, jfloatArray wVals, jintArray idx, jlongArray statsOut) {
  return gradient_sparse<jfloat, FloatElems>(env, h, wKeys, wVals, idx, statsOut, false, dsgd_gradient_sparse);
}
JNIEXPORT jint JNICALL NATIVE(gradientSparseF64)(JNIEnv* env, jobject, jlong h, jintArray wKeys, jdoubleArray wVals, jintArray idx, jlongArray statsOut) {
  return gradient_sparse<jdouble, DoubleElems>(env, h, wKeys, wVals, idx, statsOut, true, dsgd_gradient_sparse_f64);
}
JNIEXPORT jint JNICALL NATIVE(asyncStepSparse)(JNIEnv* env, jobject, jlong h, jintArray idx, jfloat lr) {
  return async_step_sparse<jfloat>(env, h, idx, lr, false, dsgd_async_step_sparse);
}
JNIEXPORT jint JNICALL NATIVE(asyncStepSparseF64)(JNIEnv* env, jobject, jlong h, jintArray idx, jdouble lr) {
  return async_step_sparse<jdouble>(env, h, idx, lr, true, dsgd_async_step_sparse_f64);
}
JNIEXPORT jint JNICALL NATIVE(getWeightsSparse)(JNIEnv* env, jobject, jlong h) {
  return get_weights_sparse<jfloat>(env, h, false, dsgd_get_weights_sparse);
}
JNIEXPORT jint JNICALL NATIVE(getWeightsSparseF64)(JNIEnv* env, jobject, jlong h) {
  return get_weights_sparse<jdouble>(env, h, true, dsgd_get_weights_sparse_f64);
}
JNIEXPORT void JNICALL NATIVE(setWeightsSparse)(JNIEnv* env, jobject, jlong h, jintArray keys, jfloatArray vals) {
  set_weights_sparse<FloatElems>(env, h, keys, vals, dsgd_set_weights_sparse);
}
JNIEXPORT void JNICALL NATIVE(setWeightsSparseF64)(JNIEnv* env, jobject, jlong h, jintArray keys, jdoubleArray vals) {
  set_weights_sparse<DoubleElems>(env, h, keys, vals, dsgd_set_weights_sparse_f64);
}
JNIEXPORT void JNICALL NATIVE(takeSparse)(JNIEnv* env, jobject, jlong h, jintArray keysOut, jfloatArray valsOut) {
  take_sparse<jfloat>(env, h, keysOut, valsOut, false);
}
JNIEXPORT void JNICALL NATIVE(takeSparseF64)(JNIEnv* env, jobject, jlong h, jintArray keysOut, jdoubleArray valsOut) {
  take_sparse<jdouble>(env, h, keysOut, valsOut, true);
}

// SlaveImpl.startAsync (core/Slave.scala:159-175): the persistent lock-free engine on ONE device-resident w
JNIEXPORT void JNICALL NATIVE(asyncStart)(JNIEnv* env, jobject, jlong h, jlongArray assignedBegin, jlongArray assignedEnd,
                                          jint batch, jfloat lr, jlong maxUpdates, jlong seed, jboolean positionalBug) {
  const jsize k = env->GetArrayLength(assignedBegin);
  if (env->GetArrayLength(assignedEnd) != k) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "assignedBegin / assignedEnd length mismatch");
    return;
  }
  int rc;
  {
    LongElems ab(env, assignedBegin, JNI_ABORT);
    LongElems ae(env, assignedEnd, JNI_ABORT);
    rc = dsgd_async_start(ctx(h), reinterpret_cast<const int64_t*>(ab.p), reinterpret_cast<const int64_t*>(ae.p), k, batch,
                          lr, maxUpdates, static_cast<uint64_t>(seed), positionalBug ? 1 : 0);
  }
  if (rc) raise(env, rc);
}

// mini-batch updates applied so far (MasterAsync counts these: core/MasterAsync.scala:83,171)
JNIEXPORT jlong JNICALL NATIVE(asyncUpdates)(JNIEnv* env, jobject, jlong h) {
  int64_t u = 0;
  int32_t running = 0;
  int rc = dsgd_async_updates(ctx(h), &u, &running);
  if (rc) raise(env, rc);
  return u;
}

// SlaveImpl.stopAsync (core/Slave.scala:187-195)
JNIEXPORT void JNICALL NATIVE(asyncStop)(JNIEnv* env, jobject, jlong h) {
  int rc = dsgd_async_stop(ctx(h));
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(asyncWait)(JNIEnv* env, jobject, jlong h) {
  int rc = dsgd_async_wait(ctx(h));
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(setWeights)(JNIEnv* env, jobject, jlong h, jfloatArray w) {
  int rc;
  {
    FloatElems wv(env, w, JNI_ABORT);
    rc = dsgd_set_weights(ctx(h), wv.p);
  }
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(getWeights)(JNIEnv* env, jobject, jlong h, jfloatArray wOut) {
  int rc;
  {
    FloatElems wv(env, wOut, 0);
    rc = dsgd_get_weights(ctx(h), wv.p);
  }
  if (rc) raise(env, rc);
}

// ---- several GPUs driven by ONE JVM thread (the dev role: master + every slave in one JVM, Main.scala:144-158) ----------
// ctxs: one context per device (create / loadCsr each), rank i = ctxs[i]; arrays over workers are context-major.
namespace {
std::vector<dsgd_ctx*> ctx_list(JNIEnv* env, jlongArray ctxs) {
  const jsize n = env->GetArrayLength(ctxs);
  std::vector<jlong> h(static_cast<size_t>(n > 0 ? n : 0));
  if (n > 0) env->GetLongArrayRegion(ctxs, 0, n, h.data());
  std::vector<dsgd_ctx*> out;
  for (jlong v : h) out.push_back(ctx(v));
  return out;
}
}  // namespace

JNIEXPORT void JNICALL NATIVE(commInitAll)(JNIEnv* env, jobject, jlongArray ctxs) {
  std::vector<dsgd_ctx*> c = ctx_list(env, ctxs);
  int rc = dsgd_comm_init_all(c.data(), static_cast<int32_t>(c.size()));
  if (rc) raise(env, rc);
}

// one process per GPU in the fp64 mode (include/dsgd.h "ACROSS RANKS"): rank 0 fills idOut (DSGD_UNIQUE_ID_BYTES bytes) and
// hands it to the other ranks over any host channel; every rank attaches its fp64 context with it
JNIEXPORT void JNICALL NATIVE(commUniqueId)(JNIEnv* env, jobject, jbyteArray idOut) {
  if (!idOut || env->GetArrayLength(idOut) != DSGD_UNIQUE_ID_BYTES) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "idOut: an array of DSGD_UNIQUE_ID_BYTES (128) bytes");
    return;
  }
  int rc;
  {
    ByteElems id(env, idOut, 0);
    rc = dsgd_comm_unique_id(reinterpret_cast<char*>(id.p));
  }
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(commInitF64)(JNIEnv* env, jobject, jlong h, jbyteArray uniqueId, jint worldSize, jint rank) {
  if (!uniqueId || env->GetArrayLength(uniqueId) != DSGD_UNIQUE_ID_BYTES) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "uniqueId: the DSGD_UNIQUE_ID_BYTES (128) bytes of commUniqueId");
    return;
  }
  int rc;
  {
    ByteElems id(env, uniqueId, JNI_ABORT);
    rc = dsgd_comm_init_f64(ctx(h), reinterpret_cast<const char*>(id.p), worldSize, rank);
  }
  if (rc) raise(env, rc);
}

// ... on Double feature values too (loadCsrF64): the communicator whose gather carries both words of every column sum
JNIEXPORT void JNICALL NATIVE(commInitF64v)(JNIEnv* env, jobject, jlong h, jbyteArray uniqueId, jint worldSize, jint rank) {
  if (!uniqueId || env->GetArrayLength(uniqueId) != DSGD_UNIQUE_ID_BYTES) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "uniqueId: the DSGD_UNIQUE_ID_BYTES (128) bytes of commUniqueId");
    return;
  }
  int rc;
  {
    ByteElems id(env, uniqueId, JNI_ABORT);
    rc = dsgd_comm_init_f64v(ctx(h), reinterpret_cast<const char*>(id.p), worldSize, rank);
  }
  if (rc) raise(env, rc);
}

JNIEXPORT void JNICALL NATIVE(commDestroy)(JNIEnv* env, jobject, jlong h) {
  int rc = dsgd_comm_destroy(ctx(h));
  if (rc) raise(env, rc);
}

// Main.scala:54-65 over the WHOLE train set: column ranking and feature counts summed over the contexts
JNIEXPORT void JNICALL NATIVE(buildDimSparsityDevices)(JNIEnv* env, jobject, jlongArray ctxs, jlongArray nTrain) {
  std::vector<dsgd_ctx*> c = ctx_list(env, ctxs);
  if (env->GetArrayLength(nTrain) != static_cast<jsize>(c.size())) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "one nTrain per context");
    return;
  }
  int rc;
  {
    LongElems nt(env, nTrain, JNI_ABORT);
    rc = dsgd_build_dim_sparsity_devices(c.data(), static_cast<int32_t>(c.size()), reinterpret_cast<const int64_t*>(nt.p));
  }
  if (rc) raise(env, rc);
}

// Master.fit batch closure (core/Master.scala:184-197) over every device of the node: idxPerWorker holds
// contexts x workersPerCtx lists; the mean runs over all of them (one all-reduce inside)
JNIEXPORT jlong JNICALL NATIVE(syncStepDevices)(JNIEnv* env, jobject, jlongArray ctxs, jobjectArray idxPerWorker,
                                               jint workersPerCtx, jfloat lr) {
  std::vector<dsgd_ctx*> c = ctx_list(env, ctxs);
  const jsize k = env->GetArrayLength(idxPerWorker);
  if (workersPerCtx < 1 || k != static_cast<jsize>(c.size()) * workersPerCtx) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "idxPerWorker must hold contexts x workersPerCtx lists");
    return 0;
  }
  std::vector<std::vector<int32_t>> lists(static_cast<size_t>(k));
  std::vector<const int32_t*> ptrs(static_cast<size_t>(k));
  std::vector<int64_t> ns(static_cast<size_t>(k));
  for (jsize i = 0; i < k; ++i) {
    jintArray a = static_cast<jintArray>(env->GetObjectArrayElement(idxPerWorker, i));
    const jsize n = a ? env->GetArrayLength(a) : 0;
    lists[i].resize(n > 0 ? n : 1);
    if (n > 0) env->GetIntArrayRegion(a, 0, n, reinterpret_cast<jint*>(lists[i].data()));
    ptrs[i] = lists[i].data();
    ns[i] = n;
    if (a) env->DeleteLocalRef(a);
  }
  dsgd_batch_stats st{};
  int rc = dsgd_sync_step_devices(c.data(), static_cast<int32_t>(c.size()), ptrs.data(), ns.data(), workersPerCtx, lr, &st);
  if (rc) raise(env, rc);
  return st.n_active;
}

JNIEXPORT jlong JNICALL NATIVE(syncStepRangesDevices)(JNIEnv* env, jobject, jlongArray ctxs, jlongArray rowBegin, jlongArray rowEnd,
                                                     jint workersPerCtx, jfloat lr) {
  std::vector<dsgd_ctx*> c = ctx_list(env, ctxs);
  const jsize k = env->GetArrayLength(rowBegin);
  if (workersPerCtx < 1 || env->GetArrayLength(rowEnd) != k || k != static_cast<jsize>(c.size()) * workersPerCtx) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "rowBegin / rowEnd must hold contexts x workersPerCtx ranges");
    return 0;
  }
  dsgd_batch_stats st{};
  int rc;
  {
    LongElems rb(env, rowBegin, JNI_ABORT);
    LongElems re(env, rowEnd, JNI_ABORT);
    rc = dsgd_sync_step_ranges_devices(c.data(), static_cast<int32_t>(c.size()), reinterpret_cast<const int64_t*>(rb.p),
                                       reinterpret_cast<const int64_t*>(re.p), workersPerCtx, lr, &st);
  }
  if (rc) raise(env, rc);
  return st.n_active;
}

// Master.localLoss / localAccuracy with the tallies summed over the contexts; out = {loss, accuracy}
JNIEXPORT void JNICALL NATIVE(lossAccDevices)(JNIEnv* env, jobject, jlongArray ctxs, jlongArray rowBegin, jlongArray rowEnd,
                                             jdoubleArray out) {
  std::vector<dsgd_ctx*> c = ctx_list(env, ctxs);
  if (env->GetArrayLength(rowBegin) != static_cast<jsize>(c.size()) || env->GetArrayLength(rowEnd) != static_cast<jsize>(c.size())) {
    env->ThrowNew(env->FindClass("java/lang/IllegalArgumentException"), "one row range per context");
    return;
  }
  double la[2] = {0, 0};
  int rc;
  {
    LongElems rb(env, rowBegin, JNI_ABORT);
    LongElems re(env, rowEnd, JNI_ABORT);
    rc = dsgd_loss_acc_devices(c.data(), static_cast<int32_t>(c.size()), reinterpret_cast<const int64_t*>(rb.p),
                               reinterpret_cast<const int64_t*>(re.p), &la[0], &la[1], nullptr);
  }
  if (rc) {
    raise(env, rc);
    return;
  }
  env->SetDoubleArrayRegion(out, 0, 2, la);
}

}  // extern "C"
