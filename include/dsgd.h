/*
 * dsgd.h -- C ABI of libdsgd_hip: the MI355X (gfx950) engine for the hot path of
 * zifeo/distributed-sgd (sparse-SVM gradient step, synchronous aggregate+update,
 * asynchronous "Hogwild" update, prediction and loss/accuracy evaluation).
 *
 * The reference has NO native/FFI interface (it is 100 % Scala on the JVM); this header is the
 * boundary the new engine introduces behind the reference's natural seams.  Every entry point
 * names the reference code whose body it replaces; citations are relative to
 * /root/reference/src/main/scala/epfl/distributed/ unless they start with "proto.proto"
 * (src/main/protobuf/proto.proto).  The JNI / ctypes stubs a maintainer would add on the
 * reference side are shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross the boundary
 *   - every function returns int: 0 = DSGD_OK, < 0 = DSGD_E*; nothing throws or aborts.
 *     dsgd_last_error() returns a thread-local message for the last failing call.
 *     (The JNI shim maps DSGD_EINVAL / DSGD_ERANGE to IllegalArgumentException /
 *     IndexOutOfBoundsException -- what `require` at math/Vec.scala:129 and
 *     math/Sparse.scala:16,63 throw -- and the rest to RuntimeException.)
 *   - dense vectors (w, g, ds, delta) have n_features + 1 float slots indexed by KEY: feature
 *     ids are 1-based (utils/Dataset.scala:30 uses the file's ids as map keys), the
 *     dimSparsity vector uses 0-based keys (Main.scala:60-62), so slot 0 and slot D both exist.
 *     "absent from the map" == 0.0f.
 *   - host buffers are owned by the caller; the library copies in / out.  Pointers ending in
 *     `_dev` are device pointers (HIP) on the context's device.
 *   - a context may be called from several host threads (the reference calls its model from an
 *     8-thread pool, utils/Pool.scala:13); calls on one context are serialised internally.
 *   - arithmetic is IEEE fp32 on the device ("fp32 CSR-SpMV gradient kernel" of BASELINE.json);
 *     the reference is fp64.  Stated tolerance: tests/test_gpu_parity.py.  A context created with
 *     DSGD_F_FP64 keeps its weights and dimSparsity in fp64 and follows the reference's (and the
 *     oracle's) fp64 trajectory for the reference's batch sizes; see "THE FP64 MODE" below and
 *     tests/test_gpu_fp64.py.
 */
#ifndef DSGD_H
#define DSGD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSGD_ABI_VERSION 1

enum {
  DSGD_OK = 0,
  DSGD_EINVAL = -1,       /* bad argument / a reference `require` would have failed            */
  DSGD_ERANGE = -2,       /* sample index outside the loaded data                              */
  DSGD_ESTATE = -3,       /* call order: no data loaded, async already running, ...            */
  DSGD_EHIP = -4,         /* HIP runtime error (message has hipGetErrorString)                 */
  DSGD_ERCCL = -5,        /* RCCL error                                                        */
  DSGD_ENOMEM = -6,
  DSGD_EUNSUPPORTED = -7  /* no gfx950 device / feature not available                          */
};

/* dsgd_config.flags: 0, or DSGD_F_FP64 (any other bit: DSGD_EINVAL, checked before the device) */
#define DSGD_F_DEFAULT 0u
#define DSGD_F_FP64 0x1u

/* THE FP64 MODE (dsgd_config.flags = DSGD_F_FP64; DESIGN.md "fp64 mode").  The reference computes in Double: an fp32
 * engine decides a row whose margin y (x . w) lies within fp32 round-off of 0 differently (core/ml/SparseSVM.scala:27-28)
 * and a constant-step run never forgets it.  An fp64 context keeps w and dimSparsity in fp64 and runs synchronous steps
 * of the reference's sizes through dsgd_cs64_step_kernel (csrc/dsgd_cs64.hpp): fp64 dots, exact 64-bit fixed-point
 * per-worker sums, the oracle's regulariser / mean / update operation for operation.
 *   Limits (a plan beyond them is refused with DSGD_EUNSUPPORTED when it is CREATED): at most 4 workers per step, at
 *   most 1,024 rows per step, and a model that fits the LDS of a slice: D <= 100,847 (1 worker), 75,631 (2),
 *   60,463 (3), 50,415 (4).  RCV1's D = 47,236 fits all four.  A step whose slice layout exceeds 1,024 slots or
 *   4,096 columns of one slice is refused as well (at creation once data and dimSparsity are there, else at the run),
 *   and so is a plan whose slice layout is larger than DSGD_CS_MAX_MB MiB: an fp64 context has no other family to run it.
 *   The existing entry points in an fp64 context:
 *   - dsgd_set_weights / dsgd_set_dim_sparsity (float): the values promoted to fp64.
 *   - dsgd_get_weights (float): the fp64 weights rounded.
 *   - dsgd_build_dim_sparsity: fp64 ds[i] = filt(1.0 / (count + 1.0)), bit for bit the oracle's; ds_out gets it rounded.
 *   - dsgd_plan_create / _n / _from_seed: the same lists and layout as fp32 (see the limits above).
 *   - dsgd_plan_run (float lr): runs with (double)lr; dsgd_plan_run_f64 takes the reference's Double.
 *   - dsgd_plan_record / dsgd_plan_read_record: the same gate bits; s_used is the fp64 s rounded.
 *   - dsgd_plan_info: vals[0] = 5 (fp64 column slices).   dsgd_grad_kernel_name: "dsgd_cs64_step_kernel".
 *   - dsgd_sync_step: a one-step fp64 plan, created, run and given back inside the call.
 *   - dsgd_forward, dsgd_loss_acc: evaluated with the fp64 weights (a float w is promoted and replaces them).
 *   - everything else that would run an fp32 training kernel returns DSGD_EUNSUPPORTED and changes nothing:
 *     dsgd_gradient, dsgd_apply, dsgd_sync_step_ranges(_async), dsgd_async_* (the float dsgd_async_step and the
 *     lock-free engine, dsgd_async_start, included), dsgd_update_grad, dsgd_comm_init, dsgd_comm_init_all,
 *     dsgd_*_devices (one thread driving several fp64 contexts is not built: see "Across ranks" below).
 *   The asynchronous iteration (Slave.asyncTask + updateGrad, core/Slave.scala:79-111,177-185; orc_async_step) has its
 *   own fp64 entry points, declared with the asynchronous path below: dsgd_async_step_f64, dsgd_update_grad_f64,
 *   dsgd_async_plan_create and dsgd_plan_run_async_f64.  They run on dsgd_cs64_async_kernel (the same plan layout,
 *   slices and exchange as the synchronous steps; the finish divides the sum by the step's rows BEFORE the
 *   regulariser), with the limits above at one worker (D <= 100,847).  An asynchronous plan is a ONE-worker plan: its
 *   step u is update first_update + u of the zero-lag schedule -- worker k = u mod K at its own iteration u div K, every
 *   update seen by every worker before the next one starts -- with the rows the lock-free engine's worker k draws at
 *   that iteration.  One deterministic schedule among those the reference allows (its own is racy).
 *   The request / response gradient and synchronous steps of ANY size have their own fp64 entry points, declared with
 *   the synchronous path below: dsgd_gradient_f64 (SlaveImpl.gradient in Double), dsgd_sync_step_f64 (any number of
 *   workers, any rows per worker, a whole split included) and dsgd_forward_f64.  They run on the row-parallel fp64
 *   family (csrc/dsgd_rp64.hpp): one 16-lane group per listed row, fp64 dots, y * x of the active rows added into
 *   64-bit fixed-point column sums with integer atomics at shift = 62 - ceil(log2 n) (n: the worker's list length,
 *   duplicates counted) relative to the data's largest |x| <= 2^vexp, so no column sum overflows and the result does not
 *   depend on the order of the list or of the adds (bit-reproducible).  EXACT RANGE: an entry of exponent e is exact on
 *   the grid when e >= vexp - (39 - ceil(log2 n)): 32 binades at n = 100, 29 at 1,024, 23 at 65,536, 21 at 214,511
 *   rows.  Inside it the results differ from the oracle's only by the rounding order of x . w and w . ds and by the
 *   oracle's per-add rounding and mid-sum 1e-20 filter, which the exact sum does not have.  OUTSIDE it (derived in
 *   oracle/bounds.py, out_of_range_bound; asserted per coordinate by tests/test_gpu_hard_values.py): an entry whose lowest
 *   mantissa bit lies below the grid unit 2^(vexp - shift) is rounded to the grid, off by at most half a unit, so a
 *   worker's sum of column j is off by at most out_j * 2^(vexp - shift - 1), out_j the number of such entries of the column
 *   in the worker's list (shift = 62 - ceil(log2 n) here, the layout's shift + 32 = 62 - ceil(log2 largest list) in the
 *   column-slice plans).  A column whose fixed-point sum is exactly 0 while its true sum is not -- certainly when every
 *   entry is below half a unit, possibly whenever the true sum is within out_j half units of 0 -- leaves the support of the sum and gets NO regulariser (math/Vec.scala:65-75): an error of |s| = |2 lambda
 *   (w . ds)| in that worker's gradient, lr / K * |s| in the weight, which is not a grid unit.  The fp32 kernels have the
 *   same two terms at the shift they report (dsgd_tuning_info).  No gate decision depends on the grid: the dots are taken
 *   on the float values as they are.  Data whose |x| spread over more than the exact range should be scaled per column,
 *   or cosine-normalised as the reference's loader does, before it is loaded.  The limits and refusals
 *   above are unchanged: dsgd_gradient, dsgd_sync_step_ranges and plans beyond them still return DSGD_EUNSUPPORTED.
 *   ACROSS RANKS (dsgd_comm_init_f64 on float feature values, dsgd_comm_init_f64v on float or Double ones; declared with
 *   the multi-GPU entry points; one process per GPU).
 *   World W ranks, each an fp64 context with its own rows, every rank calling with the same number k of hosted workers:
 *   a step is orc_sync_step over K = k * W workers in rank-major order (worker j of rank r is global worker r * k + j).
 *   Every worker's exact 64-bit column sums, its list length and its active count are gathered on every rank -- an
 *   all-gather written as ncclAllReduce(ncclInt64, ncclSum) over a buffer in which a slot is non-zero on exactly one
 *   rank, in messages of at most 1 MiB -- and every rank folds them with the single-context finish.  So after every step
 *   the replicas hold the same fp64 weights bit for bit, and those are bit for bit the weights of ONE fp64 context
 *   that holds all the rows and runs dsgd_sync_step_f64 with the K lists (row indices shifted) from the same weights.
 *   The ranks agree on what the finish depends on: ONE column ranking (column counts all-reduced), ONE vexp (the
 *   largest over the ranks' data; it stays when the communicator goes, until dsgd_load_csr) and, from
 *   dsgd_build_dim_sparsity, dimSparsity from the all-reduced feature counts -- what one process over all the train
 *   rows builds.  With a communicator attached:
 *   - dsgd_sync_step_f64, and dsgd_sync_step (float lr promoted), run that step; dsgd_batch_stats carry the job's
 *     samples and active rows on every rank.  Ranks called with different n_workers all get DSGD_EINVAL, weights
 *     unchanged (the counts travel first; a step moves K * (D + 3) * 8 bytes, rounded up to 512 per worker).
 *   - dsgd_loss_acc returns the job's loss, accuracy and counts on every rank (ranges are local rows; the tallies are
 *     summed), bit for bit a single context's over the union of the ranges.
 *   - dsgd_gradient_f64, dsgd_forward_f64, dsgd_update_grad_f64 and the get / set of weights and dimSparsity stay local.
 *   - ROW-PARALLEL PLANS RUN ACROSS THE RANKS.  dsgd_plan_create_rp64_n is accepted (local, not collective: the lists index
 *     the rank's own rows and are checked as without a communicator), and dsgd_plan_run_f64 on such a plan (dsgd_plan_run:
 *     its float lr promoted) is a COLLECTIVE call: every rank runs steps [step_begin, step_end) of its own plan, which
 *     hosts k workers, and after every step every rank holds the same bits -- those of a loop of dsgd_sync_step_f64 calls
 *     under the same communicator on the same lists, i.e. of ONE fp64 context over all the rows running dsgd_sync_steps_f64
 *     with the K = k * W lists in rank-major order.  Float and Double values (Double under dsgd_comm_init_f64v, both words
 *     gathered, as below).  The ranks agree ONCE PER CALL: before any worker's sums travel they all-reduce one word per rank
 *     (csrc/dsgd_rp64_gather.hpp rp64_call_word: k, the value type, step_end - step_begin) and the host reads them back --
 *     the call's one host read; the steps behind it are enqueued back to back (per step: the gather form of the gradient
 *     kernel, the slots' messages, a header kernel, the single context's finish; no upload, no synchronisation) and
 *     dsgd_synchronize collects the statistics, which are the JOB's samples and active rows on every rank.  Ranks that
 *     disagree on k, the value type or the number of steps all get DSGD_EINVAL with nothing changed (the weights keep
 *     their bits, the gather buffer is clean, the next matched call works); the message names the rank and what differed.
 *     An empty run (step_begin == step_end) takes part in the agreement and does nothing else.  At most 2^32 - 1 steps per
 *     call (DSGD_EINVAL before the agreement: cut the range).  A plan holds lists and nothing else: one created detached
 *     runs attached, and the other way round.  A plan whose record is switched on (dsgd_plan_record) is refused at its run
 *     with DSGD_EUNSUPPORTED while a communicator is attached.  WHAT A RANK CHECKS ALONE: the record, the 2^32 - 1 steps,
 *     k * W overflowing an int, and everything dsgd_plan_run_f64 checks without a communicator (the step range against the
 *     plan, data and dimSparsity present, a plan from before the last load) are judged from the rank's own arguments and
 *     state BEFORE the agreement, so they must hold, or fail, on every rank: a rank refused there alone has not
 *     entered the agreement, and the others wait in its all-reduce.  Only k, the value type and the number of steps are
 *     compared between the ranks.  THE STATISTICS WINDOW: the job's samples and active rows run on over the calls until
 *     dsgd_synchronize, or until the next call that writes statistics of its own (dsgd_sync_step_f64, dsgd_loss_acc, ...),
 *     whichever comes first; such a call closes the window and discards what the plan runs had counted (the weights are
 *     not affected), and a dsgd_synchronize behind it reports no rows of those runs.  Call dsgd_synchronize between a
 *     plan run and a per-step call if the run's totals matter.  A collective error inside the call returns DSGD_ERCCL and
 *     drops the gather buffer; the weights are then those behind the LAST COMPLETED STEP, as for any multi-step call (the
 *     message names it), the same on every rank only if every rank failed at the same step.
 *   - dsgd_plan_create / _n / _from_seed / _from_seed_rp64, dsgd_plan_run / _f64 on a column-slice plan,
 *     dsgd_plan_run_async_f64, dsgd_async_plan_create / _rp64, dsgd_sync_steps_f64 and dsgd_async_step_f64 return
 *     DSGD_EUNSUPPORTED and change nothing: the persistent column-slice kernel cannot hold a collective, and the device
 *     shuffle of THESE entry points and the asynchronous iteration have no form that spans the ranks -- the device shuffle
 *     that does is dsgd_plan_create_from_seed_job_rp64: a local call, accepted here, its plan run by the collective
 *     dsgd_plan_run_f64.  (host.MasterSync.fit falls back from a
 *     refused plan to one dsgd_sync_step_f64 per step; with DSGD_F64_RP_PLANS=1 to a row-parallel plan on host-drawn
 *     lists, ONE dsgd_plan_run_f64 per epoch and rank.)
 *   DOUBLE FEATURE VALUES ACROSS RANKS: a communicator attached with dsgd_comm_init_f64v is dsgd_comm_init_f64's in every
 *   rule above, and also (1) attaches with Double data loaded, (2) accepts dsgd_load_csr_f64 while attached -- the load is
 *   collective as dsgd_load_csr is: ranking and vexp are agreed at the rows' first use -- and (3) on Double data
 *   dsgd_sync_step_f64 / dsgd_sync_step gather BOTH words of every column sum (below): a worker's slot is two planes, HI
 *   with the header words and LO, one message per slot and plane, and every rank folds the K workers with the single
 *   context's Double finish -- bit for bit ONE context that holds all the rows as doubles.  A Double step moves K * 2 *
 *   (D + 3) * 8 bytes (each plane rounded up to 512): twice the float step's, the cost of the equality; LO planes are not
 *   elided.  The word that carries a rank's n_workers carries its value type too: ranks that disagree on either all get
 *   DSGD_EINVAL, weights unchanged, and the next matched step works.  Float data on every rank takes the one-word gather,
 *   bit for bit dsgd_comm_init_f64's.  dsgd_loss_acc on Double data gives the job's tallies on every rank;
 *   dsgd_sync_steps_f64, the plans listed above and dsgd_async_step_f64 stay refused as under dsgd_comm_init_f64; a
 *   row-parallel plan's run on Double data gathers both words per step as dsgd_sync_step_f64 does.
 *   Without a communicator nothing changes.  Real RCCL with more than one rank has not run; no multi-GPU speed is claimed.
 *   DOUBLE FEATURE VALUES (dsgd_load_csr_f64; csrc/dsgd_rp64.hpp).  The reference reads `elems(1).toDouble`
 *   (utils/Dataset.scala:30); dsgd_load_csr takes floats, which moves every value of a real data file by up to 6e-8
 *   relative before the first step.  dsgd_load_csr_f64 keeps the doubles (8 bytes per non-zero beside the CSR) and the
 *   values rounded to float (the column ranking and the layout code read those); vexp comes from the largest |v| as a
 *   double, and every abs(v) > 1e-20 filter that decides a result (the gradient's entries, dimSparsity's feature counts)
 *   reads the double.  dsgd_value_bits says which values are loaded (64 / 32); dsgd_load_csr brings floats back and
 *   frees the doubles.  Served on Double data, each its float-data self in statistics, state rules and errors:
 *   dsgd_gradient_f64, dsgd_gradient_sparse_f64, dsgd_sync_step_f64, dsgd_sync_step (the row-parallel step, inside the
 *   one-step plan's limits of 4 workers and 1,024 rows), dsgd_async_step_f64 / _sparse_f64 (the row-parallel pair with
 *   orc_async_step's finish, the delta in key order; the one-step plan's limits of 1,024 rows and the LDS as on float data), dsgd_forward / _f64, dsgd_loss_acc, dsgd_build_dim_sparsity,
 *   dsgd_update_grad_f64 and the get / set of weights and dimSparsity.
 *   The column sums have TWO words per column and worker.  With S = 62 - ceil(log2 n) and v = +-x * 2^(S - vexp):
 *   floor(v) goes into a signed 64-bit word HI, rn((v - floor(v)) * 2^32) into an unsigned 64-bit word LO (no carry: n
 *   <= 2^31 entries of <= 2^32), the sum is (HI * 2^32 + LO) * 2^(vexp - S - 32), rounded ONCE to double, to nearest even
 *   (csrc/dsgd_round128.hpp).  EXACT RANGE: an entry of exponent e (|x| in [2^e, 2^(e+1)), all 53 bits used) is exact
 *   when e >= vexp - (42 - ceil(log2 n)) -- 35 binades at 100 rows, 32 at 1,024, 26 at 65,536; below it an entry is
 *   off by at most half a unit 2^(vexp - S - 32).  The sums are integers: order-free and bit-reproducible.  Values a
 *   float holds exactly, inside the float grid's range, give the bits of the float-data call.
 *   Refused on Double data with DSGD_EUNSUPPORTED, nothing changed, the context usable: dsgd_plan_create / _n /
 *   _from_seed and dsgd_async_plan_create (the column-slice kernels hold 16 float values per slot in registers),
 *   dsgd_comm_init_f64, and dsgd_load_csr_f64 while a communicator of dsgd_comm_init_f64 is attached (its gather slots hold
 *   one word per column; dsgd_comm_init_f64v attaches the communicator that serves Double data: "ACROSS RANKS").
 *   host.MasterSync.fit falls back from the refused plan to dsgd_sync_step_f64 on host-drawn lists; host.MasterAsync.fit
 *   needs resident asynchronous plans and raises on Double data.
 *   AN EPOCH'S STEPS IN ONE CALL (dsgd_sync_steps_f64, declared with the synchronous path below; csrc/dsgd_rp64.hpp).
 *   Everything the plans refuse -- more than 4 workers, more than 1,024 rows per step, Double feature values -- pays
 *   dsgd_sync_step_f64's boundary once per step: a staged list, two launches, a synchronisation.  dsgd_sync_steps_f64
 *   takes a run of steps in the flat form dsgd_plan_create_n takes and IS that many dsgd_sync_step_f64 calls in order:
 *   the same bits in the weights, the loop's totals in the statistics, each step's active count on request.  One upload
 *   (the lists and their ranges), the steps enqueued without a host synchronisation between them, one synchronisation at
 *   the end.  A step is ONE launch (dsgd_rp64_step_kernel / dsgd_rp64v_step_kernel: the two bodies of the per-call step
 *   with a grid-wide arrival between them) where its grid is resident as a whole, else the per-call step's two launches;
 *   DSGD_RP64_FUSED (read at dsgd_create; 1 / 0) selects the fused form or the two-launch queue for every step.  The
 *   arrival's wait is bounded at 2 s of the device's wall clock.  A launch that gives up runs phase 2 in none of its
 *   workgroups and every later launch of the call returns on entry; no step runs behind it (a call that mixes the two
 *   forms synchronises once where it changes from fused launches to the pair).  The call then returns DSGD_ESTATE, the
 *   message names the last completed step, the weights are those behind that step, and the context is usable.
 *   dsgd_grad_kernel_name says which form served the last call's steps.  Float and Double values, any
 *   n_workers >= 1, any list lengths; the weights stay in the layout they are found in.  Refused before anything is
 *   enqueued, nothing changed, the context usable: DSGD_ESTATE on an fp32 context; DSGD_EUNSUPPORTED with a communicator
 *   attached (the lists of a call are not resident; a row-parallel plan is the epoch form there: "ACROSS RANKS");
 *   DSGD_EINVAL for null
 *   pointers, n_steps < 1, n_workers < 1, offsets that do not start at 0, decrease or do not end at n_idx, and an empty
 *   list of any step; DSGD_ERANGE for a row index outside the loaded rows in any step.
 *   ROW-PARALLEL PLANS (dsgd_plan_create_rp64_n, dsgd_plan_create_from_seed_rp64, dsgd_async_plan_create_rp64, declared
 *   behind dsgd_plan_run_async_f64; csrc/dsgd_rp64.hpp).  Everything the column-slice plans refuse had no resident form:
 *   more than 4 workers, more than 1,024 rows per step, a model beyond a slice's LDS, Double feature values.  These three
 *   creators take their twins' arguments and return an ordinary dsgd_plan* that holds only the lists and their ranges on
 *   the device.  NO layout is built: whether a run reads float or Double values is decided at each run from the data
 *   loaded then, so one plan serves both and outlives a reload between them (re-validated like any plan: DSGD_ERANGE
 *   before anything is enqueued while an index lies outside the loaded rows).  Any n_workers >= 1, any list length, any
 *   D.  _from_seed_rp64 and dsgd_async_plan_create_rp64 draw the lists of their twins entry for entry and leave the same
 *   *jstate and *draws_out; _from_seed_rp64 keeps the device shuffle's limits (DSGD_EUNSUPPORTED, *jstate untouched).
 *   dsgd_plan_run_f64 (dsgd_plan_run: its float lr promoted) enqueues, per step, the two launches of dsgd_sync_step_f64
 *   over the plan's resident ranges -- no upload, no host synchronisation; dsgd_synchronize collects the statistics --
 *   and gives bit for bit dsgd_sync_steps_f64 on the same lists, however the steps are cut into calls; the weights stay
 *   in the layout they are found in.  The fused one-launch step is NOT used: its give-up protocol needs a host read
 *   inside the call, and an enqueue-only entry point has none.  dsgd_plan_run_async_f64 (one-worker plans): per step
 *   dsgd_rp64v_s_sliced_kernel, the gradient kernel and the asynchronous finish -- on Double data bit for bit a loop of
 *   dsgd_async_step_f64 over the lists; on float data dsgd_rp64_finish_async_kernel, which also serves batches above 1,024
 *   rows and models beyond 100,847 features.  dsgd_plan_record: the documented format (bit r = row r of the step, workers
 *   in order; ceil(max_step_rows / 32) words per step; s_used = (float)s), written by dsgd_rp64_grad_rec_kernel /
 *   dsgd_rp64v_grad_rec_kernel with vector atomics into words zeroed on the stream in front of each step (a step run
 *   again overwrites its record); the weights are the bits of an unrecorded run.  In an asynchronous run s_used is the
 *   float rounding of s summed in rank order, the iteration itself uses the slice-order sum (they differ in the last bits
 *   of the double).  dsgd_plan_info: vals[0] = 6, strides 0, [7] words per step of the record.  dsgd_grad_kernel_name
 *   names the gradient kernel of the last run.  Refused, nothing changed, the context usable: DSGD_ESTATE on an fp32
 *   context; DSGD_EINVAL / DSGD_ERANGE as dsgd_sync_steps_f64 (null pointers, an empty list, offsets that are no prefix
 *   sum ending at n_idx; a row index outside the rows loaded, where data is loaded).  WITH A COMMUNICATOR ATTACHED
 *   ("ACROSS RANKS"): dsgd_plan_create_rp64_n is accepted and dsgd_plan_run_f64 / dsgd_plan_run on its plan is a collective
 *   call, one agreement and one host read per call; dsgd_plan_create_from_seed_rp64, dsgd_async_plan_create_rp64 and
 *   dsgd_plan_run_async_f64 return DSGD_EUNSUPPORTED, as does the run of a plan that keeps a record;
 *   dsgd_plan_create_from_seed_job_rp64 (the lists of a job's share of workers, drawn by the device) is accepted.  The existing
 *   creators refuse exactly as before.
 * The entry points below that name fp64 return DSGD_ESTATE on an fp32 context (dsgd_precision excepted).            */

typedef struct dsgd_ctx dsgd_ctx;

/* MODEL WIDTH.  Any D >= 1 gives the same results; what a wide model costs (measured, whole-split steps of 800,000
 * RCV1-like rows of 75 non-zeros, profiles/r06_dispatch_table.txt): the matrix is split by column frequency into the
 * 18,396 hottest columns (weights and gradient of a workgroup in LDS, 16-bit ranks in the stream) and the rest, whose
 * weights / gradient must fit ONE LDS tile of 36,796 words for the one-launch row chunks (csrc/dsgd_fstep.hpp):
 *   D <= 55,191   (RCV1: 47,236)  row chunks: 97 us per step at D = 47,236, 108 us at D = 20,000
 *   D <= 83,931                   the three streaming launches, cold columns beyond the tile gathered from L2 and added
 *                                 through 64-bit global atomics: 155 us at D = 70,000 (+ 50 %)
 *   D  > 83,931                   more than 65,536 cold columns: 32-bit cold column words (8 instead of 6 bytes per cold
 *                                 non-zero, 7.5 % of RCV1-like non-zeros), otherwise as the line above
 * dsgd_grad_kernel_name() says which family ran; tests/test_gpu_dispatch.py holds the choice to the best family.    */
typedef struct {
  int32_t n_features; /* D; 47236 for RCV1 (utils/Dataset.scala:16)                              */
  int32_t device;     /* HIP device ordinal                                                      */
  double lambda;      /* SparseSVM.lambda (core/ml/SparseSVM.scala:11; application.conf:21)      */
  uint32_t flags;
  uint32_t reserved;
} dsgd_config;

/* counters a batch call reports back (the reference increments Kamon counters per SAMPLE:
 * core/Slave.scala:131,145,90 -- the host side does counter.increment(n_samples)) */
typedef struct {
  int64_t n_samples;  /* rows whose gradient / prediction was computed                          */
  int64_t n_active;   /* rows with y * (x . w) >= 0 (core/ml/SparseSVM.scala:27-28)             */
} dsgd_batch_stats;

int dsgd_abi_version(void);
const char* dsgd_last_error(void);
/* number of visible gfx950 devices (0 if none / no HIP runtime) */
int dsgd_device_count(void);

/* ---- lifecycle: replaces `new SparseSVM(lambda, dimSparsity)` + the data array handed to
 *      `new Slave(node, master, data, model, async)` (Main.scala:68,138,148-149) ------------- */
int dsgd_create(const dsgd_config* cfg, dsgd_ctx** out);
int dsgd_destroy(dsgd_ctx* ctx);

/* data: Array[(Vec, Int)] (utils/Dataset.scala:11) as CSR.  col ids are the reference's keys (1-based feature ids),
 * each at most once per row in any order (a row is a Map: DSGD_EINVAL for a repeated key), label +1/-1.
 * Copied to HBM once; resident afterwards.  Indices in later calls refer to it,
 * exactly as GradientRequest.samples / ForwardRequest.samples index Slave.data
 * (core/Slave.scala:134,149; proto.proto:51-63).
 *
 * LOADING AGAIN.  dsgd_load_csr / dsgd_load_csr_f64 may be called on a context that holds data (not while the lock-free
 * engine runs: DSGD_ESTATE).  A successful load replaces the data and everything the library derived from it: the column
 * ranking, the split streams and their tiles, vexp and the fixed-point shifts, every cached layout of row ranges, the
 * evaluation kernels' lane group.  What stays:
 *   - the resident weights and dimSparsity, value for value in key order (dsgd_get_weights returns the bits it returned
 *     before the load); dimSparsity stays "set", i.e. it is the CALLER's to set or build again for the new rows
 *     (dsgd_set_dim_sparsity / dsgd_build_dim_sparsity) -- until then the steps use the old data's values;
 *   - every plan handle.  A plan made before the load is judged against the data loaded at its next use (dsgd_plan_run,
 *     dsgd_plan_run_f64, dsgd_plan_run_async_f64, dsgd_plan_info): if every index it holds is a row of that data it is laid
 *     out again and runs exactly as a plan created now from the same lists would; otherwise the call returns DSGD_ERANGE
 *     before anything is enqueued -- the weights untouched, the context and the plan usable, and the plan runs again after
 *     a later load under which its lists fit.  This holds for lists the library drew itself (dsgd_plan_create_from_seed,
 *     dsgd_async_plan_create: drawn inside row ranges of the data loaded THEN) as for the caller's;
 *   - under Double feature values the refusals of "THE FP64 MODE" stay as they are: no plan is created, a plan made on
 *     float data runs on the values rounded to float.  */
int dsgd_load_csr(dsgd_ctx* ctx, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_1based, const float* val,
                  const int8_t* label);
/* The same data with Double values ("THE FP64 MODE", Double feature values): fp64 contexts only (DSGD_ESTATE on an fp32
 * one), dsgd_load_csr's validation and refusals (|v| <= 3e38 as there), DSGD_EUNSUPPORTED while a communicator is
 * attached.  *bits_out of dsgd_value_bits: 64 after dsgd_load_csr_f64, 32 otherwise.                                 */
int dsgd_load_csr_f64(dsgd_ctx* ctx, int64_t n_rows, const int64_t* row_ptr, const int32_t* col_1based, const double* val,
                      const int8_t* label);
int dsgd_value_bits(dsgd_ctx* ctx, int32_t* bits_out);
int dsgd_n_rows(dsgd_ctx* ctx, int64_t* n_rows, int64_t* nnz);

/* SparseSVM.dimSparsity: either given (dense, 0-based keys as Main.scala:62 builds them) ...  */
int dsgd_set_dim_sparsity(dsgd_ctx* ctx, const float* ds /* D+1 */);
/* ... or built on the device from rows [0, n_train) exactly as Main.scala:54-65 does
 * (including the off-by-one: count of feature f lands on key f-1).  ds_out may be NULL.       */
int dsgd_build_dim_sparsity(dsgd_ctx* ctx, int64_t n_train, float* ds_out /* D+1 or NULL */);

/* resident weights (GradState.grad holds the WEIGHTS: core/ml/GradState.scala:6-10)           */
int dsgd_set_weights(dsgd_ctx* ctx, const float* w /* D+1 */);
int dsgd_get_weights(dsgd_ctx* ctx, float* w_out /* D+1 */);

/* the fp64 mode's own vectors (key order, D+1 doubles) and its precision: *bits_out = 64 or 32                   */
int dsgd_set_weights_f64(dsgd_ctx* ctx, const double* w /* D+1 */);
int dsgd_get_weights_f64(dsgd_ctx* ctx, double* w_out /* D+1 */);
int dsgd_set_dim_sparsity_f64(dsgd_ctx* ctx, const double* ds /* D+1 */);
int dsgd_get_dim_sparsity_f64(dsgd_ctx* ctx, double* ds_out /* D+1 */);
int dsgd_precision(dsgd_ctx* ctx, int32_t* bits_out);

/* ---- synchronous path ----------------------------------------------------------------------
 * SlaveImpl.gradient (core/Slave.scala:142-157): g = regularize(sum_i backward(w, x_i, y_i), w).
 * w == NULL uses the resident weights (no transfer); otherwise w (D+1 floats) replaces them,
 * like the full `weights` every GradientRequest carries (proto.proto:60-63).
 * n == 0 fails with DSGD_EINVAL (Vec.sum requires a non-empty list, math/Vec.scala:129).      */
int dsgd_gradient(dsgd_ctx* ctx, const float* w, const int32_t* idx, int64_t n, float* g_out /* D+1 */,
                  dsgd_batch_stats* stats /* may be NULL */);

/* The same three in an fp64 context ("THE FP64 MODE"; DSGD_ESTATE on an fp32 context), any list length n >= 1, with
 * the reference's Double values.  Errors as dsgd_gradient: n <= 0 or no workers DSGD_EINVAL ("Cannot sum an empty list
 * of vectors", math/Vec.scala:129); an index outside the loaded rows DSGD_ERANGE with nothing changed; refused while
 * the lock-free engine runs.  Between plan runs the weights stay in the plans' slice-major layout.
 * dsgd_gradient_f64: SlaveImpl.gradient in Double (core/Slave.scala:142-157), g = regularize(sum_i backward(w, x_i, y_i)).
 *   w == NULL uses the resident fp64 weights; otherwise w replaces them (as the GradientRequest's weights do).
 * dsgd_sync_step_f64: Master.fit's batch closure in Double (core/Master.scala:184-197), ANY number of workers and rows.
 * dsgd_forward_f64: SlaveImpl.forward with Double weights (w may be NULL): pred = -signum(x . w) in {-1, 0, +1}.      */
int dsgd_gradient_f64(dsgd_ctx* ctx, const double* w, const int32_t* idx, int64_t n, double* g_out /* D+1 */,
                      dsgd_batch_stats* stats /* may be NULL */);
int dsgd_sync_step_f64(dsgd_ctx* ctx, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers,
                       double lr, dsgd_batch_stats* stats /* may be NULL */);
int dsgd_forward_f64(dsgd_ctx* ctx, const double* w, const int32_t* idx, int64_t n, double* pred_out /* n */);
/* n_steps steps of dsgd_sync_step_f64 in one call ("AN EPOCH'S STEPS IN ONE CALL" above): step t, worker j owns
 * idx[offsets[t * n_workers + j] .. offsets[t * n_workers + j + 1]).  stats: the totals of the steps;
 * active_per_step_out[t]: step t's active rows.                                                                       */
int dsgd_sync_steps_f64(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets /* n_steps * n_workers + 1 */,
                        int64_t n_steps, int32_t n_workers, double lr, int64_t* active_per_step_out /* n_steps, may be NULL */,
                        dsgd_batch_stats* stats /* may be NULL */);

/* Master.fit batch closure, update half (core/Master.scala:194-197): w <- w - lr * g_mean      */
int dsgd_apply(dsgd_ctx* ctx, const float* g_mean /* D+1 */, float lr);

/* The whole batch closure (core/Master.scala:184-197) for n_workers workers hosted by this
 * context: per-worker regularised sums, MEAN over workers, w <- w - lr * mean.  Index lists are
 * what `split.map(Random.shuffle(_)).slice(batch, batch + batchSize)` produced on the host.
 * If a communicator is attached (dsgd_comm_init) the mean runs over n_workers * world_size
 * workers with one RCCL all-reduce of the summed gradient.
 * 40 us per call at the reference's sizes (two row-parallel launches).  Hand an epoch's lists over as ONE plan instead
 * (dsgd_plan_create / dsgd_plan_run below: 5 us per step) wherever they are known ahead -- Master.fit knows them.  With
 * DSGD_CS_REQ=1 such a request runs as ONE launch of the column-slice kernel, which lays the lists out itself
 * (csrc/dsgd_cs.hpp: dsgd_cs_request_kernel); measured SLOWER (126 us: the set-up is a latency chain), so off by default. */
int dsgd_sync_step(dsgd_ctx* ctx, const int32_t* const* idx_per_worker, const int64_t* n_per_worker,
                   int32_t n_workers, float lr, dsgd_batch_stats* stats /* may be NULL */);

/* Same, for batches that are whole contiguous row ranges (batch-size >= split size makes
 * slice(0, B) of the shuffled split the entire split; a sum does not depend on the order).
 * By the rows of the step: 512 .. 98,303 COLUMN LISTS (csrc/dsgd_tcol.hpp: the ranges' entries sorted by column once
 * per configuration; dot kernel -> one bit per row -> column-wise exact sums: no per-workgroup partials; DSGD_TCOL_MIN /
 * _MAX); beyond them ROW CHUNKS (csrc/dsgd_fstep.hpp: cold x.w, hot tiles and cold gradient of a chunk of rows in ONE
 * launch; DSGD_FSTEP_MIN); below 512 the row-wise kernel.  Layouts are cached per (ranges) configuration (eight each).
 * Every path accumulates the same fixed-point integers: same gate decisions => the same bits.                          */
int dsgd_sync_step_ranges(dsgd_ctx* ctx, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers,
                          float lr, dsgd_batch_stats* stats /* may be NULL */);

/* Asynchronous launch variants: enqueue on the context's stream and return; results/errors are
 * collected by dsgd_synchronize().  steps x workers index lists live in a resident plan so that
 * no host->device traffic happens between steps (timed loops, hipGraph replay).                 */
typedef struct dsgd_plan dsgd_plan;
/* idx: concatenation of all lists; offsets: n_steps * n_workers + 1 prefix offsets into idx.
 * A plan is RESIDENT and laid out for the device WHEN IT IS CREATED (data and dimSparsity present; otherwise at its first
 * run), by the device itself, on a stream of its own beside the launch stream: dsgd_plan_create returns once the lists are
 * staged and one 16-byte read-back has fixed the layout's strides; the rest of the set-up overlaps whatever the launch
 * stream is running (the next epoch's plan can be created while this epoch's steps run).  Steps of the reference's own size
 * (<= 8 hosted workers, <= 1,024 rows per step: application.conf:15,27) become COLUMN SLICES -- dsgd_plan_run then runs
 * ALL steps of [step_begin, step_end) in ONE persistent launch (5 us per 3 x 100 step, 9 us per 4 x 200; a launch of a
 * single step 11 us: hand over as many steps per call as are known); larger steps are laid out over the device's streams
 * (16 bytes per 8 non-zeros) and, up to DSGD_VT_PACK_MB (default 2048), copied in that order: two launches per step
 * (18 us at 4,096 rows).  One epoch of Master.fit (core/Master.scala:179-199) = one plan: the device blocks of a destroyed
 * plan are kept by the context for the next one (DSGD_CACHE_MB, default 8192), dsgd_plan_destroy does not synchronise.
 * The same lists through dsgd_sync_step (per request) cost 40 us per call.                                            */
int dsgd_plan_create(dsgd_ctx* ctx, const int32_t* idx, const int64_t* offsets, int64_t n_steps, int32_t n_workers,
                     dsgd_plan** out);
/* The same with the length of idx stated: DSGD_EINVAL unless offsets[n_steps * n_workers] == n_idx -- the form a binding
 * that holds idx as a managed array must use (the lists are read up to offsets[last]: a JVM array shorter than that
 * would be read past its end).  The JNI shim, the Python binding and include/dsgd.hpp all go through this one.       */
int dsgd_plan_create_n(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps,
                       int32_t n_workers, dsgd_plan** out);
/* One EPOCH of Master.fit as a plan whose lists are DRAWN BY THE DEVICE, draw for draw the reference's random stream
 * (core/Master.scala:184: for every batch every worker's whole split is reshuffled -- scala.util.Random.shuffle over
 * java.util.Random -- and sliced; 1.38 G draws per epoch of RCV1 at full = true, which a host reproduces in 0.19 s on 32
 * threads while the epoch's 2,146 steps run in 10 ms).  *jstate is java.util.Random's 48-bit internal state (what
 * `new java.util.Random(seed)` holds: (seed ^ 0x5DEECE66D) & (2^48 - 1)) in front of the epoch's first draw; on success it
 * is the state behind the last draw of the steps emitted (*draws_out raw values later), exactly as the JVM's generator
 * would stand.  split k = rows [split_begin[k], split_end[k]) (SplitStrategy.vanilla, the caller's); the steps are those of
 * `0 until max_samples by batch_size` up to the first one that hands some worker an EMPTY slice (*n_steps_out of them: the
 * reference's slave throws there, math/Vec.scala:129; 0 steps: *out = NULL).  csrc/dsgd_shuffle.hpp: the raw stream is
 * scanned for rejection candidates by every lane of the device at once, the host walks the ~10^5 candidates (the one
 * sequential part), and every (batch, worker) list is traced backwards through its Fisher-Yates by one workgroup straight
 * into the plan's index buffer.  DSGD_EUNSUPPORTED (nothing drawn, *jstate untouched): batch_size > 1,024, a split of more
 * than 2^20 rows, or a stream outside the device form's limits -- draw the lists on the host then (the Python / C++ host
 * mirrors do: csrc/jrand.c) and use dsgd_plan_create_n.  The practical ceiling is below the 2^20 rows: a shuffle of len rows
 * rejects len^2 / 2^33 raw values on average and the device form holds 64 per shuffle, so from roughly 600,000 rows per
 * split on almost every epoch is refused (one shuffle in its thousands exceeds 64) and at 2^20 rows (128 expected) all are.
 * dsgd_plan_create_from_seed_job below lifts the three limits (any batch size, 512 rejections, a rank's window of a job).
 * tests/test_gpu_shuffle.py, tests/test_gpu_shuffle_large.py: equal to csrc/jrand.c entry for entry.                         */
int dsgd_plan_create_from_seed(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end,
                               int32_t n_splits, int64_t max_samples, int32_t batch_size, dsgd_plan** out,
                               int64_t* n_steps_out, int64_t* draws_out);
/* The same epoch for A JOB'S SHARE OF WORKERS, at any batch size.  The reference's stream is ONE stream over all workers
 * of the job (core/Master.scala:184): for every batch b = 0, B, 2B, ... < max_samples and for every job worker j in the
 * master's order one Random.shuffle of job_len[j] entries is drawn and its slice [b, b + B) taken; the steps end at the
 * first b at which ANY job worker's split is exhausted.  This context hosts job workers first .. first + n_local - 1: the
 * plan holds their n_steps x n_local lists (step-major, worker-minor), hosted worker i mapping position p of its shuffle to
 * row split_begin[i] + p of the rows loaded HERE (split_begin has n_local entries and need not follow the job's order).
 * *jstate advances over ALL the job's draws and *draws_out is the job's total, whatever the window: every rank of a job
 * leaves with the same generator state, the one csrc/jrand.c leaves after dsgd_jrand_epoch_lists over the n_job splits.
 * With first = 0 and n_local = n_job the lists, step count, state and draws are those of dsgd_plan_create_from_seed / _rp64
 * wherever that form accepts the arguments.
 *   Limits: any batch_size >= 1 (a list is traced in chunks of 1,024 entries, each sweeping the steps above it: about
 *   ceil(B / 1,024) x (len - b) draw evaluations per list); every job_len[j] in 1 .. 2^20; up to 512 rejected raw values
 *   inside one shuffle (128 +- 11 expected at 2^20 rows).  Beyond them DSGD_EUNSUPPORTED: nothing drawn, *jstate
 *   untouched, *out = NULL, *n_steps_out = 0.  DSGD_EINVAL: null pointers, n_job < 1, n_local < 1, first < 0,
 *   first + n_local > n_job, a job_len < 1, a negative split_begin.  DSGD_ERANGE: a hosted split ends beyond the rows loaded.
 *   The fp32 form refuses Double data, the _rp64 form needs an fp64 context (float or Double data), as their twins do.
 *   UNDER A COMMUNICATOR both are local calls with no collective: the fp32 form is accepted under dsgd_comm_init, the
 *   _rp64 form under dsgd_comm_init_f64 / _f64v, and its plan runs through the collective dsgd_plan_run_f64 as a
 *   host-drawn row-parallel plan does.  EVERY RANK MUST PASS THE SAME *jstate, job_len, max_samples, batch_size AND n_local
 *   (its own `first` and split_begin): nothing here compares them across ranks -- the collective run checks the number of
 *   workers and the step count as it does for any plan.  (dsgd_plan_create_from_seed_rp64 stays refused there.)
 * tests/test_gpu_seed_job.py, tests/test_gpu_seed_job_world2.py: equal to csrc/jrand.c entry for entry.                     */
int dsgd_plan_create_from_seed_job(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first,
                                   int32_t n_local, const int64_t* split_begin, int64_t max_samples, int32_t batch_size,
                                   dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out);
int dsgd_plan_create_from_seed_job_rp64(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first,
                                        int32_t n_local, const int64_t* split_begin, int64_t max_samples, int32_t batch_size,
                                        dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out);
/* the lists of a plan as the device holds them: the first n entries and the first n_offsets prefix offsets (tests) */
int dsgd_plan_read_lists(dsgd_ctx* ctx, dsgd_plan* plan, int32_t* idx_out, int64_t n, int64_t* offsets_out, int64_t n_offsets);
int dsgd_plan_destroy(dsgd_ctx* ctx, dsgd_plan* plan);
/* The device blocks destroyed plans leave with the context (up to DSGD_CACHE_MB, default 8192 MiB, read at dsgd_create;
 * a block no plan took again within ~5 plans is freed by itself): give back all but keep_bytes of them now (blocks the
 * launch stream is still reading stay); *held_out (may be NULL) = bytes still held.  For hosts that run several
 * contexts on one GPU (the dev role's JVM workers, Main.scala:144-158) and want the memory between fits.            */
int dsgd_cache_trim(dsgd_ctx* ctx, int64_t keep_bytes, int64_t* held_out);
int dsgd_plan_run(dsgd_ctx* ctx, dsgd_plan* plan, int64_t step_begin, int64_t step_end, float lr);
/* the same in an fp64 context, with the reference's Double learning rate (DSGD_ESTATE on an fp32 context)           */
int dsgd_plan_run_f64(dsgd_ctx* ctx, dsgd_plan* plan, int64_t step_begin, int64_t step_end, double lr);
/* How a plan will run (nothing in the reference; benchmarks, tests): vals[0] = 1 column slices (dsgd_cs_step_kernel),
 * 2 the one-workgroup kernel, 3 virtual tiles, 4 the row-parallel kernels, 5 fp64 column slices, 6 a row-parallel fp64
 * plan (dsgd_plan_create_rp64_n and its kin: strides 0), 7 a logistic plan (dsgd_plan_create_lg_n, dsgd_plan_create_from_seed_lg:
 * strides 0), 8 a logistic plan on column slices (dsgd_plan_create_lg_cs_n, dsgd_plan_create_from_seed_lg_cs while their
 * layout is current: dsgd_lg_cs_step_kernel, [1] = 16), 0 not laid out yet; [1] slices, [2..4] slot /
 * row / column-list strides, [5] slots per lane, [6] 1 if the device laid it out, [7] words per step of the record,
 * [8] lanes per slice workgroup (512; 256 where DSGD_CS_NT=256 took: [5] is 2 for that kernel and the wide two-slot one).
 * n <= 9 slots.                                                                                                       */
int dsgd_plan_info(dsgd_ctx* ctx, dsgd_plan* plan, int32_t* vals, int32_t n);
/* Parity aid for LONG synchronous runs (nothing in the reference; tests/test_gpu_cs_device.py, tests/test_gpu_host.py, tests/test_sync_replay.py, bench.py): with the record
 * on, every step a column-slice plan runs leaves the GATE DECISION of each of its rows (bit r of the step's words: row r
 * of the step -- workers in order, each worker's list in order -- had y (x . w) >= 0, core/ml/SparseSVM.scala:27-28) and
 * the regulariser scalar s = 2 lambda (w . ds) it used (SparseSVM.scala:31).  fp32 against fp64 decides a row on the gate
 * differently once in a few thousand steps and a constant-step run then goes its own way; with the engine's decisions on
 * record the oracle REPLAYS the trajectory exactly (oracle/sync_replay.py): the final weights must agree to rounding, and
 * every decision that differs from the oracle's own must be a row whose margin lies inside the fp32 bound.
 * dsgd_plan_record(on = 0) drops the record.  dsgd_plan_read_record copies the words of steps [step_begin, step_end)
 * (*mask_words_out words each; gate_mask / s_used may be NULL to query the width).                                    */
int dsgd_plan_record(dsgd_ctx* ctx, dsgd_plan* plan, int32_t on);
int dsgd_plan_read_record(dsgd_ctx* ctx, dsgd_plan* plan, int64_t step_begin, int64_t step_end, uint32_t* gate_mask,
                          float* s_used, int32_t* mask_words_out);
int dsgd_sync_step_ranges_async(dsgd_ctx* ctx, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers,
                                float lr);
int dsgd_synchronize(dsgd_ctx* ctx, dsgd_batch_stats* stats_accum /* may be NULL */);

/* ---- evaluation --------------------------------------------------------------------------
 * SlaveImpl.forward (core/Slave.scala:129-140): pred_i = -signum(x_i . w) in {-1, 0, +1}       */
int dsgd_forward(dsgd_ctx* ctx, const float* w /* or NULL */, const int32_t* idx, int64_t n, float* pred_out /* n */);

/* Master.localLoss / localAccuracy (core/Master.scala:100-107; core/ml/SparseSVM.scala:16-23)
 * over rows [row_begin, row_end): loss = lambda*|w|^2 + mean_i max(0, 1 - y_i p_i), acc =
 * mean_i [p_i == y_i].  counts (may be NULL) gets the exact integer tallies
 * {#p==y, #p==0, #p==-y}.  With a communicator attached, tallies are summed over ranks.        */
int dsgd_loss_acc(dsgd_ctx* ctx, const float* w /* or NULL */, int64_t row_begin, int64_t row_end, double* loss,
                  double* acc, int64_t* counts /* 3 or NULL */);

/* Master.predict / distributedLoss / distributedAccuracy (core/Master.scala:61-98) for the workers hosted by this
 * context, in ONE launch (csrc/dsgd_predict.hpp).  The reference splits the rows over the workers, sends each a
 * ForwardRequest (core/Slave.scala:129-140: pred_i = -signum(x_i . w)), zips the replies back to the rows and folds
 * loss and accuracy over the resulting map.  Here range k = rows [row_begin[k], row_end[k]) is worker k's split:
 *   pred_out     one int8 in {-1, 0, +1} per row, range-major: row row_begin[k] + t is at off[k] + t, off the prefix
 *                sums of the range lengths.
 *   counts_out   (may be NULL) 3 exact tallies per range, {#p==y, #p==0, #p==-y} as dsgd_loss_acc counts them.
 *   loss, acc    (may be NULL) with n all rows and c the tallies summed over the ranges:
 *                loss = lambda*|w|^2 + (c1 + 2 c2) / n, acc = c0 / n -- dsgd_loss_acc's expression and |w|^2.
 * A row's prediction and its tally are decided on the same x . w, computed as the row-wise evaluation kernel of the
 * context's precision computes it (and as dsgd_forward / dsgd_forward_f64 do: the predictions are theirs, entry for
 * entry).  So the counts of a range are the ones dsgd_loss_acc returns for the same rows and weights in an fp64 context,
 * and in an fp32 context for ranges below 4,096 rows; from 4,096 rows on the fp32 dsgd_loss_acc streams the split matrix
 * with another summation order of x . w, and a row within fp32 rounding of x . w = 0 may be counted differently there.
 * An empty range (begin == end) is an empty reply: no bytes, zero tallies.  DSGD_EINVAL, nothing changed: n_ranges < 1
 * or > 256, begin > end, ranges that overlap (the reference's .toMap would collapse repeated rows and preds.size would
 * no longer be the row count; SplitStrategy.vanilla never overlaps), no rows at all (.reduce over an empty map
 * throws, :96).  Rows outside the loaded data: DSGD_ERANGE, nothing changed.  While the lock-free engine runs the call
 * is refused with DSGD_ESTATE (its concurrent loss check is dsgd_loss_acc).
 * w == NULL uses the resident weights; otherwise w replaces them, under dsgd_forward's / dsgd_forward_f64's rules.
 * dsgd_predict_ranges on an fp64 context takes w == NULL only (the resident Double weights; a float w is DSGD_EINVAL:
 * Double weights go through dsgd_predict_ranges_f64, which needs an fp64 context, DSGD_ESTATE otherwise).
 * LOCAL to the rank: no collective is entered whether or not a communicator is attached; predictions, tallies, loss
 * and accuracy cover this context's rows only (dsgd_loss_acc is the call that sums tallies over ranks).           */
int dsgd_predict_ranges(dsgd_ctx* ctx, const float* w /* D+1 or NULL */, const int64_t* row_begin, const int64_t* row_end,
                        int32_t n_ranges, int8_t* pred_out /* sum of lengths */, int64_t* counts_out /* 3 * n_ranges or NULL */,
                        double* loss /* may be NULL */, double* acc /* may be NULL */);
int dsgd_predict_ranges_f64(dsgd_ctx* ctx, const double* w /* D+1 or NULL */, const int64_t* row_begin, const int64_t* row_end,
                            int32_t n_ranges, int8_t* pred_out, int64_t* counts_out, double* loss, double* acc);

/* Master.localSampledLoss / localSampledAccuracy (core/Master.scala:109-118): loss and accuracy folded over
 *   Random.shuffle(workingData.indices) take samplesCount map workingData
 * in ONE launch over rows already resident (csrc/dsgd_eval_list.hpp).  Two forms:
 *
 * dsgd_loss_acc_list evaluates the n >= 1 rows idx names.  A row named twice is counted twice (`map workingData`
 * keeps duplicates; the sampled form never produces any).  An entry outside the loaded rows: DSGD_ERANGE, no output
 * written.  With c the exact tallies {#p==y, #p==0, #p==-y} (counts, may be NULL):
 *   loss = lambda*|w|^2 + (c1 + 2 c2) / n, acc = c0 / n -- dsgd_loss_acc's expression and its |w|^2 (either may be NULL).
 * A row is decided on the x . w that dsgd_predict_ranges decides it on, so the tallies are the ones folded from
 * dsgd_forward / dsgd_forward_f64 over the same list, and for idx = row_begin .. row_end - 1 the ones dsgd_loss_acc
 * returns, under the condition dsgd_predict_ranges states (fp64: always; fp32: below 4,096 rows).
 *
 * dsgd_loss_acc_sampled draws the list itself, on the device, draw for draw the reference's stream: *jstate is
 * java.util.Random's 48-bit state in front of the shuffle's first draw and, on success, the state behind its last;
 * *draws_out (may be NULL) the raw values consumed, rejections included.  With len = row_end - row_begin the list is
 * the first n = min(samples_count, len) entries (the reference's `take`; *n_out, may be NULL) of
 * Random.shuffle(0 until len), entry p naming row row_begin + p; idx_out (n entries, may be NULL) receives the rows --
 * the list does not visit the host otherwise.  One shuffle with its slice [0, n) is a one-worker, one-step job of
 * dsgd_plan_create_from_seed_job, and its limits hold: len up to 2^20 rows and at most 512 rejections inside the
 * shuffle.  Beyond them DSGD_EUNSUPPORTED: nothing is drawn, *jstate is untouched, nothing is written -- draw with
 * dsgd_jrand_shuffle (csrc/jrand.c) and use the list form.  len == 1 draws nothing and evaluates that row.
 *
 * DSGD_EINVAL, nothing written or drawn: null ctx / idx / jstate, n < 1, samples_count < 1, row_begin >= row_end (the
 * reference's .reduce over an empty sample throws; the JVM would have spent the shuffle's draws before throwing, this
 * call does NOT).  A window outside the loaded rows: DSGD_ERANGE.  While the lock-free engine runs: DSGD_ESTATE.
 * w == NULL uses the resident weights; otherwise w replaces them, under dsgd_predict_ranges' / _f64's rules: the float
 * forms on an fp64 context take w == NULL only (DSGD_EINVAL otherwise), the _f64 forms need an fp64 context
 * (DSGD_ESTATE otherwise).
 * LOCAL to the rank: no collective is entered whether or not a communicator is attached.                          */
int dsgd_loss_acc_list(dsgd_ctx* ctx, const float* w /* D+1 or NULL */, const int32_t* idx, int64_t n, double* loss, double* acc,
                       int64_t* counts /* 3 or NULL */);
int dsgd_loss_acc_list_f64(dsgd_ctx* ctx, const double* w /* D+1 or NULL */, const int32_t* idx, int64_t n, double* loss, double* acc,
                           int64_t* counts /* 3 or NULL */);
int dsgd_loss_acc_sampled(dsgd_ctx* ctx, const float* w /* D+1 or NULL */, uint64_t* jstate, int64_t row_begin, int64_t row_end,
                          int64_t samples_count, double* loss, double* acc, int64_t* counts /* 3 or NULL */,
                          int32_t* idx_out /* min(samples_count, row_end - row_begin) rows or NULL */, int64_t* n_out,
                          int64_t* draws_out);
int dsgd_loss_acc_sampled_f64(dsgd_ctx* ctx, const double* w /* D+1 or NULL */, uint64_t* jstate, int64_t row_begin, int64_t row_end,
                              int64_t samples_count, double* loss, double* acc, int64_t* counts, int32_t* idx_out, int64_t* n_out,
                              int64_t* draws_out);

/* ---- asynchronous ("Hogwild") path ---------------------------------------------------------
 * one iteration of Slave.asyncTask (core/Slave.scala:92-101) on the resident weights with the
 * given sample list: grad = MEAN_i backward; delta = lr * regularize(grad, w); w -= delta.
 * delta_out (D+1, may be NULL) receives what Slave.scala:103-105 would gossip.                 */
int dsgd_async_step(dsgd_ctx* ctx, const int32_t* idx, int64_t n, float lr, float* delta_out,
                    dsgd_batch_stats* stats /* may be NULL */);

/* SlaveImpl.updateGrad / MasterAsync.updateGrad / GradState.update
 * (core/Slave.scala:177-185, core/MasterAsync.scala:164-177, core/ml/GradState.scala:8):
 * w[key[i]] -= dv[i].  Keys as in the wire message Sparse.map (proto.proto:28-31); a key outside [0, D] fails with
 * DSGD_ERANGE before anything is applied.  May be called WHILE the lock-free engine runs (the reference's handler runs
 * concurrently with asyncTask): the update is applied with atomic adds on a side stream and folded into the engine's
 * regulariser scalar; the call returns when it has been applied and never waits for the engine.                    */
int dsgd_update_grad(dsgd_ctx* ctx, const int32_t* key, const float* dv, int64_t nnz);
/* The same in an fp64 context ("THE FP64 MODE"; DSGD_ESTATE on an fp32 context), with the reference's Double values.
 * dsgd_async_step_f64: one iteration on the resident fp64 weights (a one-step, one-worker plan, run and given back inside
 * the call); delta_out (D+1 doubles, key order, may be NULL) receives lr * regularize(mean) -- zero off the support.
 * dsgd_update_grad_f64: w[k] = filt(w[k] - dv) for each key, then the whole vector filtered; synchronous (the update is
 * applied when it returns).  The keys are checked on the host first: a key outside [0, D] gives DSGD_ERANGE, a repeated
 * key DSGD_EINVAL (a Sparse delta has unique keys); w is unchanged then.
 * dsgd_async_plan_create: a one-worker plan of n_updates steps whose lists the DEVICE draws -- step u holds the rows of
 * update first_update + u of the zero-lag schedule (see "THE FP64 MODE"), the lock-free engine's sampler for the workers'
 * row ranges [assigned_begin[k], assigned_end[k]), `batch`, `seed` and `positional_bug` (as dsgd_async_start).
 * dsgd_plan_run_async_f64: the asynchronous iterations [step_begin, step_end) of a one-worker plan (DSGD_EINVAL for a
 * plan of more workers); dsgd_plan_record / dsgd_plan_read_record serve these runs as they serve synchronous ones.      */
int dsgd_async_step_f64(dsgd_ctx* ctx, const int32_t* idx, int64_t n, double lr, double* delta_out /* D+1, may be NULL */,
                        dsgd_batch_stats* stats);
int dsgd_update_grad_f64(dsgd_ctx* ctx, const int32_t* key, const double* dv, int64_t nnz);
int dsgd_async_plan_create(dsgd_ctx* ctx, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers,
                           int32_t batch, uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates,
                           dsgd_plan** out);
int dsgd_plan_run_async_f64(dsgd_ctx* ctx, dsgd_plan* plan, int64_t step_begin, int64_t step_end, double lr);
/* Row-parallel plans ("THE FP64 MODE", ROW-PARALLEL PLANS): the arguments of dsgd_plan_create_n,
 * dsgd_plan_create_from_seed and dsgd_async_plan_create; fp64 contexts only, float or Double data, any number of workers,
 * any list length, any D.  The plan runs through dsgd_plan_run / _f64 / _async_f64 like any other.                    */
int dsgd_plan_create_rp64_n(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets, int64_t n_steps,
                            int32_t n_workers, dsgd_plan** out);
int dsgd_plan_create_from_seed_rp64(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end,
                                    int32_t n_splits, int64_t max_samples, int32_t batch_size, dsgd_plan** out,
                                    int64_t* n_steps_out, int64_t* draws_out);
int dsgd_async_plan_create_rp64(dsgd_ctx* ctx, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers,
                                int32_t batch, uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates,
                                dsgd_plan** out);

/* ---- SPARSE VALUES at the boundary (csrc/dsgd_sparse.hpp) --------------------------------------
 * The reference exchanges Sparse{map<int32, double>, size} values only (proto.proto:28-31) and stores no entry with
 * abs(v) <= 1e-20 (math/Sparse.scala:104-118).  These forms take and return exactly that -- parallel arrays of keys and
 * values -- so that no caller builds, copies or scans D + 1 slots.  Each is its dense twin (dsgd_set_weights /
 * dsgd_get_weights / dsgd_gradient / dsgd_async_step and their _f64 forms) in results, side effects, statistics, state
 * rules and errors: the same kernels compute the gradient, the values are bit for bit the twin's.
 *   Output: the pairs with |(double)v| > 1e-20, keys ASCENDING, *nnz_out of them (-0.0, 0.0 and anything at or under the
 *   threshold are dropped).  cap is the room in the two output arrays.  cap too small in a PURE form
 *   (dsgd_get_weights_sparse*, dsgd_gradient_sparse*): DSGD_EINVAL, *nnz_out = the count needed, the arrays untouched --
 *   call again.  dsgd_async_step_sparse* change the weights, so a delta must never be lost: they are refused with
 *   DSGD_EINVAL BEFORE anything runs unless cap >= min(D + 1, the listed rows' lengths summed) -- the delta's support lies
 *   inside the union of the listed rows' columns (the regulariser is support-only, math/Vec.scala:65-75).  cap = D + 1
 *   always qualifies.
 *   Input: nnz pairs, every key once and inside [0, D], in any order; nnz == 0 is the zero vector.  The keys are checked on
 *   the host before anything moves: a key outside [0, D] DSGD_ERANGE, a repeated key DSGD_EINVAL, the weights unchanged.
 *   fp32 values are stored as dsgd_set_weights stores them, fp64 values as dsgd_set_weights_f64 does (both drop
 *   abs(v) <= 1e-20).  w_nnz < 0 in the gradient forms: the resident weights (no transfer).
 *   Precision: the float forms behave on an fp64 context as their twins do (dsgd_set_weights_sparse promotes,
 *   dsgd_get_weights_sparse rounds, dsgd_gradient_sparse and dsgd_async_step_sparse DSGD_EUNSUPPORTED); the _f64 forms
 *   return DSGD_ESTATE on an fp32 context.  While the lock-free engine runs they are refused where their twins are
 *   (dsgd_get_weights_sparse stays allowed).  One host synchronisation per call, as the twins have.                  */
/* w <- the Sparse value {key -> val}, 0 elsewhere (GradientRequest.weights / StartAsyncRequest.weights, proto.proto:51-70) */
int dsgd_set_weights_sparse(dsgd_ctx* ctx, const int32_t* key, const float* val, int64_t nnz);
int dsgd_set_weights_sparse_f64(dsgd_ctx* ctx, const int32_t* key, const double* val, int64_t nnz);
/* the resident weights as a Sparse value, keys ascending (GradState.grad, core/ml/GradState.scala:6-10) */
int dsgd_get_weights_sparse(dsgd_ctx* ctx, int32_t* key_out, float* val_out, int64_t cap, int64_t* nnz_out);
int dsgd_get_weights_sparse_f64(dsgd_ctx* ctx, int32_t* key_out, double* val_out, int64_t cap, int64_t* nnz_out);
/* SlaveImpl.gradient (core/Slave.scala:142-157) with Sparse in and out.  w_nnz < 0: the resident weights. */
int dsgd_gradient_sparse(dsgd_ctx* ctx, const int32_t* w_key, const float* w_val, int64_t w_nnz, const int32_t* idx, int64_t n,
                         int32_t* g_key, float* g_val, int64_t cap, int64_t* g_nnz, dsgd_batch_stats* stats /* may be NULL */);
int dsgd_gradient_sparse_f64(dsgd_ctx* ctx, const int32_t* w_key, const double* w_val, int64_t w_nnz, const int32_t* idx, int64_t n,
                             int32_t* g_key, double* g_val, int64_t cap, int64_t* g_nnz, dsgd_batch_stats* stats /* may be NULL */);
/* one iteration of Slave.asyncTask (core/Slave.scala:92-105) with the delta it gossips as a Sparse value */
int dsgd_async_step_sparse(dsgd_ctx* ctx, const int32_t* idx, int64_t n, float lr, int32_t* d_key, float* d_val, int64_t cap,
                           int64_t* d_nnz, dsgd_batch_stats* stats /* may be NULL */);
int dsgd_async_step_sparse_f64(dsgd_ctx* ctx, const int32_t* idx, int64_t n, double lr, int32_t* d_key, double* d_val, int64_t cap,
                               int64_t* d_nnz, dsgd_batch_stats* stats /* may be NULL */);

/* SlaveImpl.startAsync (core/Slave.scala:159-175) for n_workers lock-free workers sharing ONE
 * device-resident weight vector: every worker (a workgroup) loops
 *   draw `batch` of its assigned rows -> mean gated gradient on a snapshot -> regularize ->
 *   atomicAdd(w[j], -lr * g_j)
 * until dsgd_async_stop or until max_updates mini-batch updates have been applied in total
 * (MasterAsync counts UPDATES, maxSteps = N * maxEpochs: core/MasterAsync.scala:83,171).
 * assigned_begin/end: worker k samples rows [assigned_begin[k], assigned_end[k]) (the
 * SplitStrategy.vanilla ranges); sampling is `shuffle take batch` (Slave.scala:87) or a single
 * uniform draw when batch == 1 (Slave.scala:84).  positional_bug != 0 reproduces
 * Slave.scala:87's indexing of `data` by POSITION (rows 0 .. n_k-1) instead of by assigned id. */
int dsgd_async_start(dsgd_ctx* ctx, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers,
                     int32_t batch, float lr, int64_t max_updates, uint64_t seed, int32_t positional_bug);
int dsgd_async_updates(dsgd_ctx* ctx, int64_t* updates, int32_t* running);
/* Asynchronous mode ACROSS GPUs: with a communicator attached, every context runs its own
 * single-w engine on its own rows and the replicas exchange updates every `every_updates` LOCAL mini-batch updates:
 * one all-reduce of what each replica subtracted since the last exchange, after which every replica subtracts its
 * peers' part -- the batched form of the reference's gossip (core/Slave.scala:103-105 sends every update to every
 * peer, :177-185 / core/MasterAsync.scala:164-177 subtract it).  0 (default) = no exchange.  Every rank must use
 * the same period and the same finite max_updates (the ranks enqueue the same number of collectives).            */
int dsgd_async_set_exchange(dsgd_ctx* ctx, int64_t every_updates);
int dsgd_async_stop(dsgd_ctx* ctx); /* SlaveImpl.stopAsync, core/Slave.scala:187-195 */
/* Measurement aid (nothing in the reference).  counters (4, may be NULL): mini-batch updates applied, rows whose
 * gradient was computed, rows the gate let through, lane-level atomicAdd(w[j], -delta_j) performed (SURVEY.md 8(d):
 * "additionally report atomics/s").  s_engine / s_exact (may be NULL): the engine's incrementally kept regulariser scalar
 * s = 2 lambda (w . ds) as the device holds it (one atomic add per mini-batch and per dsgd_update_grad call, re-derived
 * from the weights every few thousand iterations), and the same quantity recomputed from the weights as they are now.
 * While the engine runs the two differ by the updates in flight; counters [1..3] are flushed by every worker each 16 of
 * its iterations and when it leaves: exact once the engine is joined, up to 16 mini-batches per worker behind before
 * (counters[0], what MasterAsync polls, is exact at any time).                                                      */
int dsgd_async_stats(dsgd_ctx* ctx, int64_t* counters, double* s_engine, double* s_exact);
int dsgd_async_wait(dsgd_ctx* ctx); /* block until max_updates reached */
/* MasterAsync's loss check on ONE weight snapshot (core/MasterAsync.scala:109-138: loss, accuracy, bestGrad and the update
 * count all come from one innerGradState).  While the lock-free engine runs, dsgd_loss_acc and dsgd_get_weights each see
 * the weights at another moment; these three calls see one copy of them (csrc/dsgd_snapshot.hpp).  fp32 contexts without
 * a communicator; allowed while the engine runs and while it does not.
 * dsgd_async_check: copies the resident weights into a device buffer (every weight read once, as the engine reads it),
 * and returns loss and accuracy OF THAT COPY over rows [row_begin, row_end): loss = lambda |snap|^2 + (c1 + 2 c2) / n,
 * acc = c0 / n with the tallies counts = {#p==y, #p==0, #p==-y} (loss, acc, counts may be NULL) -- dsgd_loss_acc's
 * expression, kernels and summation orders, so on a context at rest the two calls agree bit for bit.  updates_window
 * (may be NULL) = {lo, hi}, update counts read around the copy: every update with a commit number <= lo is contained in
 * the snapshot WHOLE (an update's additions are drained before its number is drawn); an update with a larger number may
 * be contained in part, those above hi included (an update in flight adds before it has a number); hi is the count read
 * behind the last weight.  With no engine running lo = hi = dsgd_async_updates.  One host synchronisation; the engine's
 * stream is never touched.
 * dsgd_async_check_keep: the last check's snapshot becomes the best one (two handles change places: no kernel, no copy).
 * dsgd_async_check_weights: the last check's snapshot (which = 0) or the kept one (which = 1) in key order, D + 1 floats;
 * neither call touches the live weights.
 * Errors, with nothing enqueued and nothing changed: DSGD_EINVAL for a null context or w_out, an empty range, which
 * outside {0, 1}; DSGD_ERANGE for rows outside the data; DSGD_ESTATE with no data or no dimSparsity, for _keep without a
 * check and for _weights without the snapshot asked for since the last dsgd_load_csr (a load changes the internal
 * column order and drops both); DSGD_EUNSUPPORTED on an fp64 context (its asynchronous schedule runs no concurrent
 * engine: dsgd_loss_acc is consistent there) and with a communicator attached (dsgd_loss_acc sums over the ranks).    */
int dsgd_async_check(dsgd_ctx* ctx, int64_t row_begin, int64_t row_end, double* loss, double* acc,
                     int64_t* counts /* 3 or NULL */, int64_t* updates_window /* {lo, hi} or NULL */);
int dsgd_async_check_keep(dsgd_ctx* ctx);
int dsgd_async_check_weights(dsgd_ctx* ctx, int32_t which /* 0 last, 1 best */, float* w_out /* D+1, key order */);
/* Parity aid for the MANY-worker lock-free engine (nothing in the reference; tests/test_gpu_hogwild_trace.py, bench.py):
 * with a trace of `capacity` records attached (0 detaches it), every mini-batch update of the following engine runs
 * leaves one record at index (its commit number - 1): the worker that made it, that worker's iteration number (the key
 * of the engine's replayable sampler), the update count its weights were read at, the regulariser
 * scalar s = 2 lambda (w . ds) it used, and the GATE DECISIONS of its mini-batch (bit t of the mask = row t of the
 * sample was active, core/ml/SparseSVM.scala:27-28).  A constant-step lock-free run is chaotic -- no replay that
 * re-decides the gates can follow it -- but with the engine's own decisions on record the oracle recomputes every update
 * exactly (oracle/hogwild_replay.py): the final weights must agree to rounding, and the recorded decisions are held
 * to the margins of the replayed weights at `read_at`.  A many-worker parity statement that can fail.
 * dsgd_async_read_trace copies the first min(n, recorded) records of the LAST run out (engine joined); gate_mask holds
 * *mask_words_out = ceil(batch / 32) words per record; *n_out = records available (both may be NULL; n = 0 queries them). */
int dsgd_async_set_trace(dsgd_ctx* ctx, int64_t capacity);
int dsgd_async_read_trace(dsgd_ctx* ctx, int32_t* worker, uint32_t* iteration, int64_t* read_at, float* s_used,
                          int32_t* n_active, uint32_t* gate_mask, int64_t n, int64_t* n_out, int32_t* mask_words_out);
/* ... and what every recorded decision was TAKEN ON (round 6): dots holds *batch_out floats per record, entry t = the
 * fp32 x . w row t of the update's sample was gated on; seen_from[i] <= read_at[i] is an update count read (returning
 * atomic) before the iteration requested any weight: every update with a commit number <= seen_from had fully landed in
 * the weights the iteration saw (0 for a launch's first iteration: only the run's starting weights are known to be in).
 * With these the oracle checks EVERY decision of a run of any worker count (oracle/hogwild_replay.gate_check_recorded_dots):
 * decision == !(y d < 0) for the recorded d (core/ml/SparseSVM.scala:27-28), and d inside the range x . w can take over
 * the replayed weights between seen_from and the updates still in flight at the commit (core/Slave.scala:92).       */
int dsgd_async_read_trace_dots(dsgd_ctx* ctx, int64_t* seen_from, float* dots, int64_t n, int32_t* batch_out);

/* ---- multi-GPU (one process per GPU) ---------------------------------------
 * The synchronous master's aggregate (core/Master.scala:190-194: Future.sequence barrier +
 * Vec.mean) becomes ONE ncclAllReduce(sum, float, D+1) over xGMI on the context's stream.
 * unique_id is the 128-byte ncclUniqueId produced on rank 0 and distributed by the host
 * (torch.distributed / MPI / files).                                                           */
#define DSGD_UNIQUE_ID_BYTES 128
int dsgd_comm_unique_id(char* id_out /* DSGD_UNIQUE_ID_BYTES */);
int dsgd_comm_init(dsgd_ctx* ctx, const char* unique_id, int32_t world_size, int32_t rank);
int dsgd_comm_destroy(dsgd_ctx* ctx);
/* The same for an fp64 context ("THE FP64 MODE", "Across ranks"; DSGD_ESTATE on an fp32 context -- dsgd_comm_init keeps
 * refusing an fp64 one with DSGD_EUNSUPPORTED).  A collective call: every rank attaches in the same state (its rows
 * loaded, or not yet).  Loaded rows are ranked again here, from the column counts summed over the ranks, and the ranks
 * agree on vexp; rows loaded later at their first use, as in fp32.  dsgd_comm_destroy detaches.                      */
int dsgd_comm_init_f64(dsgd_ctx* ctx, const char* unique_id, int32_t world_size, int32_t rank);
/* dsgd_comm_init_f64 for Double feature values ("ACROSS RANKS", Double feature values across ranks): the same call and the
 * same communicator, accepted with dsgd_load_csr_f64's data loaded and accepting that load while attached; steps on Double
 * data gather both words of the column sums.  On float data everything is dsgd_comm_init_f64's, bit for bit.          */
int dsgd_comm_init_f64v(dsgd_ctx* ctx, const char* unique_id, int32_t world_size, int32_t rank);
/* The communicator the LOGISTIC model's steps span ("THE LOGISTIC MODEL", ACROSS RANKS): fp32 contexts only (an fp64 one:
 * DSGD_EUNSUPPORTED), at most 64 ranks; dsgd_comm_init's argument checks.  The SVM's entry points behave as under
 * dsgd_comm_init.  A collective call: every rank attaches in the same state; loaded rows are ranked again here from the column
 * counts summed over the ranks, rows loaded later at their first use.  dsgd_comm_destroy detaches.                     */
int dsgd_comm_init_lg(dsgd_ctx* ctx, const char* unique_id, int32_t world_size, int32_t rank);

/* ---- several GPUs driven by ONE host thread --------------------------------------------------------------------
 * The reference's dev role runs the master and every slave in ONE JVM (Main.scala:144-158); SURVEY.md 8(b) lists the
 * fused step as dsgd_sync_step(ctx, idx_per_dev, n_per_dev, lr).  A collective blocks its caller until every rank has
 * joined, so one thread cannot call the per-context entry points one after the other; these take all the contexts of
 * the node at once (one context per device, every one with its own rows): each context's kernels in front of a
 * collective are enqueued first, then all the collectives inside one ncclGroupStart / ncclGroupEnd, then what follows
 * -- the kernels, sums and summation order of N processes with one GPU each (replicas bit-identical).
 * Arrays over workers are context-major: worker k of context i at [i * workers_per_ctx + k].                       */
int dsgd_comm_init_all(dsgd_ctx* const* ctxs, int32_t n_ctx);   /* rank i = ctxs[i]; replaces dsgd_comm_unique_id + dsgd_comm_init */
/* column ranking + dimSparsity with both counts summed over the contexts (Main.scala:54-65 over the whole train set)  */
int dsgd_build_dim_sparsity_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int64_t* n_train_per_ctx);
int dsgd_sync_step_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int32_t* const* idx_per_worker,
                           const int64_t* n_per_worker, int32_t workers_per_ctx, float lr, dsgd_batch_stats* stats /* summed; may be NULL */);
int dsgd_sync_step_ranges_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int64_t* row_begin, const int64_t* row_end,
                                  int32_t workers_per_ctx, float lr, dsgd_batch_stats* stats /* summed; may be NULL */);
/* Master.localLoss / localAccuracy over rows [row_begin[i], row_end[i]) of every context, tallies summed               */
int dsgd_loss_acc_devices(dsgd_ctx* const* ctxs, int32_t n_ctx, const int64_t* row_begin, const int64_t* row_end, double* loss,
                          double* acc, int64_t* counts /* 3 or NULL */);

/* ---- introspection for benchmarks ---------------------------------------------------------
 * average device time (ms) of the dominant gradient kernel over its launches since the last
 * reset, measured with HIP events on the launch stream; n_launches may be NULL.               */
int dsgd_prof_enable(dsgd_ctx* ctx, int32_t on /* 0 off, 1 all profiled kernels, 2 the dominant kernel only */);
int dsgd_prof_read(dsgd_ctx* ctx, double* grad_kernel_ms_avg, int64_t* n_launches, int32_t reset);
/* Split layout only: average duration (ms) and launch count of {main gradient kernel, cold x.w kernel, cold
 * gradient kernel} since the last reset of dsgd_prof_read.  Measurement aid; nothing in the reference. */
int dsgd_prof_read_kinds(dsgd_ctx* ctx, double* ms_avg3, int64_t* n_launches3);

/* Non-zeros of rows [row_begin, row_end) as held internally (empty rows count one explicit zero), and how many of
 * them live in the cold stream of the split layout (0 in the other layouts).  Used by bench.py to attribute the
 * algorithmic bytes of a step to the kernel that reads them.  Nothing in the reference. */
int dsgd_range_nnz(dsgd_ctx* ctx, int64_t row_begin, int64_t row_end, int64_t* nnz, int64_t* cold_nnz);

/* Tuning state that changes numerics or layout, for benchmark records and the derived error bound of the tests:
 * vals[0] = layout generation (4 = matrix split by column rank, the only one), [1] = hot/cold split rank, [2] =
 * fixed-point shift of the last gradient launch (whole ranges and index lists alike; not the one-workgroup plan
 * kernel, which derives 30 - ceil(log2 batch) per batch), [3] = 1 if the cold stream is packed, [4] = 1 if small
 * batches run in the persistent plan kernel, [5] = 1 if the data-dependent fixed-point bound is enabled, [6] = how often
 * the row chunks of the last chunked launch's configuration have been re-cut by their workgroups' measured durations (0-2;
 * only with DSGD_FSTEP_REBALANCE=1: measured at 1 %, off by default -- the re-cut moves rows between workgroups, it changes no bit of any sum),
 * [7] = lanes per row of the fp32 row-wise evaluation kernels (dsgd_forward, dsgd_predict_ranges, dsgd_loss_acc_list /
 * _sampled, dsgd_async_check, dsgd_loss_acc below 4,096 rows) for the loaded data: 8, 16, 32 or 64 from the mean
 * non-zeros per row (above 12: 16, above 96: 32, above 192: 64; over the non-zeros as dsgd_n_rows reports them, where
 * a row without a non-zero counts one), chosen by dsgd_load_csr[_f64]; 16 before any data is loaded.  The width fixes the order in which a row's products are added, nothing else; the fp64 kernels always use 16.
 * n = number of slots the caller provides (<= 8).                                                                 */
int dsgd_tuning_info(dsgd_ctx* ctx, int32_t* vals, int32_t n);

/* Layout introspection (tests of the multi-GPU path): the internal frequency rank of every key, D + 1 entries.  With a
 * communicator attached the ranking is derived from the column counts summed over the ranks: identical on all of them. */
int dsgd_column_ranks(dsgd_ctx* ctx, int32_t* rank_of_key /* D+1 */);

/* Tuning aid (DSGD_PLAN_PROF=1 in the environment at dsgd_create): shader-clock cycles thread 0 of the small-batch
 * plan kernel spent in the nine phases of a batch ([0..8]: gather+dot, barrier, gate+tables, barrier, scatter,
 * barrier, requests, sweep, barrier+collect) and the number of steps ([15]), accumulated since the last reset;
 * 16 words, all zeros when the aid is off.                                                                       */
int dsgd_debug_cycles(dsgd_ctx* ctx, uint64_t* out16, int32_t reset);

/* name of the gradient kernel variant in use (for matching rocprofv3 kernel-trace rows)        */
const char* dsgd_grad_kernel_name(dsgd_ctx* ctx);
/* raw device pointers (float[D+1], the library's internal column order: dsgd_column_ranks) for hosts that own the
 * collective (e.g. torch.distributed).  The call brings the resident weights into that vector (a column-slice run keeps
 * them slice-major elsewhere until some entry point needs them): *w_dev is current for work enqueued on *stream until the
 * next dsgd_plan_run / dsgd_sync_step; ask again after those.                                                          */
int dsgd_device_ptrs(dsgd_ctx* ctx, void** w_dev, void** g_dev, void** stream);

/* ---- K8: dense logistic mini-batch step (BASELINE.json configs[4]) ------------------------------------------
 * NO REFERENCE COUNTERPART: the reference has one model, the sparse hinge "SVM" (core/ml/SparseSVM.scala:11;
 * Main.scala:67 "could use another model").  This is the optional dense variant north_star names: a second, small
 * object next to dsgd_ctx.  X is n_rows x D fp32 row-major in HBM (D a multiple of 512, <= 8192), labels in {0, 1}:
 *   z = X w, p = sigmoid(z), loss = mean(softplus(z) - y z), g = X^T (p - y) / B, w <- w - lr g
 * over the contiguous rows [row_begin, row_end) of the (pre-shuffled) shard -- one mini-batch.  With a communicator
 * the gradient sums are all-reduced and B is the global batch.  Oracle: oracle/dense_ref.py (fp64, pinned by finite
 * differences -- parity unpinned by construction).
 *
 * INDEX LISTS.  The _list forms, dsgd_dense_predict_list and the plans take a mini-batch as a list of row numbers
 * instead: position k of the list names row idx[k], a row named twice counts twice, and a list may be longer than
 * n_rows -- so the shard is loaded once, in any order, and every epoch draws new batches from it.  A list step is,
 * operation for operation, the range step over a shard holding the named rows in list order: the same weights, bit
 * for bit (a block of the kernel is 8 -- matrix cores: 16 -- consecutive list POSITIONS; csrc/dsgd_dense.hpp).
 * Lists are host memory.  Every check runs on the host before anything is enqueued or changed, and a refused call
 * leaves the weights as they were: DSGD_EINVAL for a null pointer, n < 1, an empty step of a plan, offsets that do not
 * run non-decreasing from 0 to n_idx, or a bad step range; DSGD_ERANGE for an entry outside [0, n_rows), naming entry
 * and position; DSGD_ESTATE without data.  With a communicator every rank passes a list of the same length.         */
typedef struct dsgd_dense dsgd_dense;
int dsgd_dense_create(int32_t n_features, int32_t device, dsgd_dense** out);
int dsgd_dense_destroy(dsgd_dense* d);
/* synthetic shard generated on the device: x ~ N(0,1)/sqrt(D), y = [x . w* + noise > 0]; the planted w* is the same
 * for every seed (one problem, many shards), the seed (= rank) varies the rows and the label noise                  */
int dsgd_dense_generate(dsgd_dense* d, int64_t n_rows, uint64_t seed);
/* host-provided data (tests): X n_rows x D row-major, y n_rows                                                    */
int dsgd_dense_load(dsgd_dense* d, int64_t n_rows, const float* X, const float* y);
int dsgd_dense_set_weights(dsgd_dense* d, const float* w /* D */);
int dsgd_dense_get_weights(dsgd_dense* d, float* w_out /* D */);
/* one mini-batch step, enqueued on the object's stream (dsgd_dense_synchronize collects)                          */
int dsgd_dense_step(dsgd_dense* d, int64_t row_begin, int64_t row_end, float lr);
int dsgd_dense_synchronize(dsgd_dense* d);
/* mean logistic loss and accuracy of the resident weights over rows [row_begin, row_end) (no update)               */
int dsgd_dense_loss(dsgd_dense* d, int64_t row_begin, int64_t row_end, double* loss, double* acc);
int dsgd_dense_comm_init(dsgd_dense* d, const char* unique_id, int32_t world_size, int32_t rank);
/* average device time (ms) of the step kernel since the last reset (HIP events on the object's stream)             */
int dsgd_dense_prof(dsgd_dense* d, int32_t enable, double* kernel_ms_avg, int64_t* n_launches);
/* dsgd_dense_step over the rows a list names; enqueued like it.  The list is copied before the call returns: calls
 * issued back to back without dsgd_dense_synchronize each use their own list.                                       */
int dsgd_dense_step_list(dsgd_dense* d, const int32_t* idx, int64_t n, float lr);
/* dsgd_dense_loss over the rows a list names                                                                        */
int dsgd_dense_loss_list(dsgd_dense* d, const int32_t* idx, int64_t n, double* loss, double* acc);
/* p = sigmoid(x . w) of every row of a range / of every position of a list, under the resident weights (no update)  */
int dsgd_dense_predict(dsgd_dense* d, int64_t row_begin, int64_t row_end, float* p_out /* row_end - row_begin */);
int dsgd_dense_predict_list(dsgd_dense* d, const int32_t* idx, int64_t n, float* p_out /* n */);
/* An epoch's lists resident on the device: step s is idx[offsets[s] .. offsets[s + 1]), uploaded once here.
 * dsgd_dense_plan_run enqueues steps [step_begin, step_end) -- each a dsgd_dense_step_list of its list -- with no
 * upload and no host synchronisation in between.  A plan belongs to the object it was created on (dsgd_dense_destroy
 * releases what is left) and to the data resident at its creation: after a dsgd_dense_load / dsgd_dense_generate its
 * run is refused with DSGD_ESTATE.  dsgd_dense_prof counts list steps and plan steps as it counts range steps.       */
typedef struct dsgd_dense_plan dsgd_dense_plan;
int dsgd_dense_plan_create(dsgd_dense* d, const int32_t* idx, int64_t n_idx, const int64_t* offsets /* n_steps + 1 */,
                           int64_t n_steps, dsgd_dense_plan** out);
int dsgd_dense_plan_run(dsgd_dense* d, dsgd_dense_plan* plan, int64_t step_begin, int64_t step_end, float lr);
int dsgd_dense_plan_destroy(dsgd_dense* d, dsgd_dense_plan* plan);

/* ---- THE LOGISTIC MODEL on the resident CSR rows (csrc/dsgd_logistic.hpp) ----------------------
 * A second linear model beside the gated hinge SVM, on the rows, the labels and the weights an fp32 context holds
 * (the reference's model seam "could use another model", Main.scala:67).  New symbols only: no SVM entry point
 * changes, DSGD_ABI_VERSION stays 1.
 *
 * THE SIGN CONVENTION IS THE TEXTBOOK'S, NOT THE SVM'S.  With d = x . w:  P(y = +1 | x) = sigma(d) and the class is
 * signum(d) in {-1, 0, +1} -- dsgd_forward and dsgd_loss_acc beside it predict -signum(d) (SparseSVM.scala:14).
 * Weights trained by one model score the other's labels upside down.
 *
 *   labels       y in {-1, +1} as loaded
 *   d = x . w    the fp32 engine's own dot: its fixed lane order, its 1e-20 product filter.  A finite d is a
 *                precondition, as for the SVM
 *   loss         l = log(1 + exp(-y d)), evaluated as max(-a, 0) + log1p(exp(-|a|)), a = y d, in fp64;
 *                reported: lambda |w|^2 + mean_i l_i  (the lambda |w|^2 of the reference's loss, SparseSVM.scala:20-23)
 *   gradient     c_i x_i per row, c_i = sigma(d_i) - (1 + y_i) / 2 = -y_i / (1 + exp(y_i d_i)), in fp64 from the fp32
 *                d_i: no NaN for a finite d (exp -> inf gives -+0, exp -> 0 gives -y)
 *   regulariser  plain L2: + 2 lambda w_j on EVERY column, per worker -- the exact gradient of the reported loss.
 *                dimSparsity plays no part: these calls work whether or not it has been set
 *   step         the reference's flow (Master.scala:184-197): a worker's regularised gradient is a SUM over its rows,
 *                the MEAN is taken over the K workers, w <- w - lr mean.  Per column j in fp64:
 *                G_k = acc_k 2^(vexp - S_k), r_k = G_k + 2 lambda w_j, the r_k added in worker order, / K,
 *                w_j' = (float)(w_j - lr mean): ONE rounding to float per step
 *   sums         a worker's list of n rows (duplicates count) uses S = 62 - ceil(log2 n); an entry adds
 *                rn(c_i x_ij 2^(S - vexp)) as a 64-bit integer (2^vexp >= max |x|, |c| <= 1: no column sum leaves its
 *                word).  Integer adds do not depend on order: a step's weights are bit-reproducible whatever the
 *                list's order, the launch's shape or the run; dsgd_lg_sync_step_ranges gives the bits of
 *                dsgd_lg_sync_step on the ranges' rows as lists, dsgd_lg_sync_steps those of its steps one by one
 *   statistics   n_samples is the number of rows, n_active EQUALS n_samples: every row contributes (there is no gate)
 *
 * Refusals -- every check runs on the host before anything is enqueued; a refused call leaves the weights as they
 * were and the context usable:
 *   DSGD_EINVAL        a null pointer; n < 1; no workers; an empty worker list; offsets that do not run from 0 to
 *                      n_idx without decreasing, or an empty list among them; an empty or reversed range
 *   DSGD_ERANGE        an index (or a range's end) outside the loaded rows
 *   DSGD_ESTATE        no data loaded, or the lock-free engine is running
 *   DSGD_EUNSUPPORTED  an fp64 context, or a communicator attached by anything but dsgd_comm_init_lg ("ACROSS RANKS" below)
 *
 * RESIDENT PLANS.  dsgd_plan_create_lg_n (the arguments of dsgd_plan_create_n; dsgd_lg_sync_steps' checks on the host before
 * anything is staged) and dsgd_plan_create_from_seed_lg (the arguments, limits, refusals and *jstate / *n_steps_out /
 * *draws_out of dsgd_plan_create_from_seed: the device draws the epoch's lists from the reference's stream) make a
 * LOGISTIC plan: the lists and their ranges resident, no layout (as a row-parallel fp64 plan).  dsgd_plan_run on it
 * enqueues, per step, the two launches of dsgd_lg_sync_step over the resident lists -- no upload, no host synchronisation;
 * the weights get the bits of dsgd_lg_sync_steps on the same lists.  dsgd_synchronize reports the rows run, n_active ==
 * n_samples.  dimSparsity is not asked for.  dsgd_plan_info: vals[0] = 7, strides 0.  dsgd_plan_read_lists and
 * dsgd_plan_destroy as for any plan.  Refused before anything is enqueued: what every call here refuses (above);
 * dsgd_plan_run_f64, dsgd_plan_run_async_f64, dsgd_plan_record and dsgd_plan_read_record on such a plan
 * (DSGD_EUNSUPPORTED); a plan from before a dsgd_load_csr whose lists no longer fit the rows (DSGD_ERANGE at the run).
 *
 * COLUMN SLICES (opt-in).  dsgd_plan_create_lg_cs_n and dsgd_plan_create_from_seed_lg_cs take the arguments and make the
 * checks and refusals of dsgd_plan_create_lg_n and dsgd_plan_create_from_seed_lg; the logistic plan they make additionally
 * has its column slices laid out (the SVM plans' device builder, on the build stream, into blocks of the plan cache that the
 * plan owns).  dsgd_plan_run on it is then ONE launch of dsgd_lg_cs_step_kernel for the whole range of steps: 16 persistent
 * workgroups, each keeping the weights of the frequency ranks r = b (mod 16) and one int64 accumulator per hosted worker and
 * column in LDS; per step one exchange of the rows' partial x.w through the SVM family's tagged granules (the same bounded
 * wait: a launch that gives up is reported by dsgd_synchronize as DSGD_ESTATE, the weights as the launch found them), the
 * scatter of rn(x c 2^(S_k - vexp)) into the accumulators, and dsgd_lg_sync_step's finish on EVERY column of the slice.
 * dsgd_plan_info: vals[0] = 8; dsgd_grad_kernel_name: "dsgd_lg_cs_step_kernel".
 *   numerics   x.w is the sum of 16 slice partials (a slot of <= 16 products in sequence, a row's slots in order, the
 *              slices in order), not the row form's lane order: the weights are NOT the bits of dsgd_lg_sync_steps.  They are
 *              a function of the lists and the starting weights alone -- the same for one run or the same steps split over
 *              several, for caller lists or device-drawn ones -- and stay within tests/logistic_cs_bound.py of the fp64 model.
 *   declines   16 slices need (1 + 2 K) words of LDS per column: at D + 1 = 47,237 that serves K <= 6 hosted workers
 *              (csrc/dsgd_lg_cs_host.hpp: lg_cs_pick_G).  A plan with more workers, a step of more than 1,024 rows or with more
 *              than 1,024 slots or 4,096 columns in one slice, a model of fewer than 64 columns, a layout the plan cache
 *              cannot hold (DSGD_CS_MAX_MB), or a layout from before a dsgd_load_csr: the plan is created and runs all the same,
 *              as a plan of dsgd_plan_create_lg_n does -- vals[0] = 7, the bits of dsgd_lg_sync_steps.
 *   state      the run leaves no |w'|^2 words: the next logistic evaluation computes them, as for weights set by the caller.
 *              The exchange buffer and its tag counter are the SVM slice plans': both kinds may run in turn on one context.
 *   otherwise  everything RESIDENT PLANS says: n_active == n_samples, dimSparsity not asked for, the same refusals.
 *
 * dsgd_lg_loss_acc_ranges: dsgd_lg_loss_acc over n_ranges <= 16 row ranges (they may overlap or repeat) in ONE launch
 * with ONE synchronisation -- an epoch's train and test passes.  loss_out[r] and acc_out[r] (either may be NULL) are the
 * bits of dsgd_lg_loss_acc on range r alone: every range has its own workgroups, the grid of a launch of its own.
 * DSGD_EINVAL: more than 16 ranges, none, an empty or reversed range; DSGD_ERANGE: a range that leaves the rows.
 *
 * WHOLE-SPLIT STEPS BY COLUMN LISTS.  dsgd_lg_sync_steps_ranges runs n_steps steps over the SAME K row ranges in one call: the
 * weights, the |w'|^2 words and the statistics (n_samples = n_active = the rows of ONE step) are the bits of n_steps calls of
 * dsgd_lg_sync_step_ranges.  The first call over a ranges configuration lays the ranges' entries out by (worker, column) on
 * the device (8 bytes per entry; at most eight configurations stay cached per context, the least recently used one makes
 * room, a dsgd_load_csr drops them all); a step is then three launches -- a coefficient per row, the gradient column by
 * column without an atomic per non-zero, the finish of every logistic step -- with no host synchronisation between steps
 * and one at the end.  The sums are the same 64-bit integers, so nothing depends on which form ran.  Where no layout can be
 * had (2^31 entries or more, 2^31 rows or more in the ranges together, no memory) the steps run as dsgd_lg_sync_step_ranges'
 * do and the call still succeeds; dsgd_grad_kernel_name says "dsgd_lg_cgrad_kernel" or "dsgd_lg_grad_range_kernel".
 * Refusals: those of dsgd_lg_sync_step_ranges with its codes, and n_steps < 1 (DSGD_EINVAL).  No other call takes this path.
 *
 * ACROSS RANKS (dsgd_comm_init_lg, declared with the multi-GPU entry points; one process per GPU; csrc/dsgd_lg_gather.hpp,
 * DESIGN.md 7.5).  A worker's column sums are integers, so they cross the ranks without rounding.  Under this communicator
 * dsgd_lg_sync_step, dsgd_lg_sync_step_ranges, dsgd_lg_sync_steps_ranges, dsgd_lg_sync_steps and dsgd_plan_run on a plan of
 * dsgd_plan_create_lg_n (whose creation stays local) are COLLECTIVE: every rank calls with the same k hosted workers and the
 * same number of steps, on its own shard (row indices are the shard's).  Global worker r * k + j is rank r's worker j.  The
 * weights on every rank are the bits of ONE context that holds shard 0 || shard 1 || ... and steps those K = k * world lists or
 * ranges in that order; the statistics are the job's rows (a plan's through dsgd_synchronize).
 *   agreement  once per call, in front of the first launch: the ranks all-reduce a record of (k, steps, the vexp of the own
 *              data) and read it back -- the call's one extra host read.  Ranks that differ in k or in the steps ALL return
 *              DSGD_EINVAL, weights unchanged, and the next agreed call works.  The call runs on the LARGEST vexp, the one a
 *              single context computes on all the rows; the context's own vexp is not changed.  A rank that fails a check of
 *              its OWN arguments returns without joining: the callers keep the ranks' arguments valid together
 *   a step     the gradient kernels sum into the rank's own slots of the K; one ncclAllReduce(int64, sum) over the slots and
 *              one length word per worker is the exact all-gather; every rank folds the K workers in worker order with the
 *              single context's finish arithmetic.  Several steps of one call are enqueued without host synchronisation
 *   local      dsgd_lg_gradient, dsgd_lg_predict, dsgd_lg_loss_acc and dsgd_lg_loss_acc_ranges enter no collective: the shard,
 *              the shard's own vexp, the figures of a context without a communicator (the caller combines the ranks');
 *              likewise dsgd_lg_predict_ranges, dsgd_lg_loss_acc_list and dsgd_lg_loss_acc_sampled (below)
 *   lists      dsgd_plan_create_from_seed_job_lg: a rank's window of the JOB's device-drawn lists -- the arguments, limits,
 *              refusals and *jstate / *n_steps_out / *draws_out of dsgd_plan_create_from_seed_job (ONE stream over all n_job
 *              workers, the lists of workers first .. first + n_local - 1, any batch size), on an fp32 context with float
 *              values, into a logistic plan (dsgd_plan_info: 7, nothing laid out).  A LOCAL call: accepted without a
 *              communicator and under this one; dsgd_plan_run on the plan is the collective run of dsgd_plan_create_lg_n's.
 *              With first = 0 and n_local = n_job the lists, the step count, the state and the draws are those of
 *              dsgd_plan_create_from_seed_lg wherever that form accepts the arguments.  There is no column-slice twin
 *   the job's  dsgd_lg_eval_job (COLLECTIVE): this rank's n_local row ranges take the positions rank * n_local + j of a job of
 *   evaluation K = n_local * world <= 256 ranges (the global worker order of the steps; without a communicator world = 1).  On
 *              EVERY rank counts_out (3 K), range_loss_out (K), loss and acc are bit for bit what dsgd_lg_predict_ranges
 *              returns on ONE context that holds the ranks' rows in rank order, for those K ranges and the same weights: a
 *              range's workgroups, tree and row order depend on the range and the device alone, the ranking under this
 *              communicator is the job's, and the |w|^2 words are the same on every replica.  Local checks first (those of
 *              dsgd_lg_predict_ranges on the local ranges, with its codes); then the agreement above with n_local in k's place
 *              (ranks that differ, or a rank in a step beside one in an evaluation: DSGD_EINVAL everywhere, nothing ran); ONE
 *              launch of dsgd_lg_predict_ranges_kernel, dsgd_lg_eval_fold_kernel (csrc/dsgd_lg_eval_job.hpp: per range three
 *              tallies, the fp64 bit pattern of its sum of l_i, a writer count), ONE in-place ncclAllReduce(int64, sum) of
 *              pad64(5 K) words -- an exact all-gather -- one read-back, and dsgd_lg_predict_ranges' fold in position order.
 *              A position not written by exactly one rank: DSGD_ESTATE.  w == NULL: the resident weights, else w replaces
 *              them; the call leaves weights, accumulators and the cached |w|^2 words as dsgd_lg_predict_ranges does.  Classes
 *              and probabilities are not gathered (dsgd_lg_predict_ranges gives a rank its own rows')
 *   refused    DSGD_EUNSUPPORTED, weights untouched: dsgd_plan_create_from_seed_lg (the whole-job form is one process's:
 *              dsgd_plan_create_from_seed_job_lg is the form for ranks), dsgd_plan_create_lg_cs_n,
 *              dsgd_plan_create_from_seed_lg_cs, and dsgd_plan_run on a column-slice plan made before the attach.  Under
 *              dsgd_comm_init and on contexts joined by dsgd_comm_init_all every logistic call stays refused
 *   errors     a collective that fails half way: DSGD_ERCCL, the buffer is dropped (dsgd_lg_eval_job: its record's buffer),
 *              the weights are those behind the last completed step
 * After dsgd_comm_destroy the calls are local again.  Real RCCL with more than one rank has not run; no speed is claimed.
 *
 * DISTRIBUTED AND SAMPLED EVALUATION (csrc/dsgd_lg_eval.hpp; ref: core/Master.scala:61-118) -- what dsgd_predict_ranges,
 * dsgd_loss_acc_list and dsgd_loss_acc_sampled are to the SVM, with the logistic model's sign, loss and fixed-order sums.
 *
 * dsgd_lg_predict_ranges: Master.predict / distributedLoss / distributedAccuracy over n_ranges <= 256 disjoint row ranges
 * (the workers' splits) in ONE launch with ONE synchronisation.  Every row is decided ONCE, on one d = x . w:
 *   class_out       (may be NULL) one int8 per row, range-major (row row_begin[r] + t at off[r] + t, off the prefix sums of
 *                   the lengths): signum(d) -- +1, -1, or 0 for d == +-0: the TEXTBOOK sign, not the SVM's.
 *   proba_out       (may be NULL) sigma(d) per row, range-major: the bits of dsgd_lg_predict over the same rows.  class_out[t]
 *                   is the sign of the d behind proba_out[t]: p > 0.5 means +1, p < 0.5 means -1.
 *   counts_out      (may be NULL) 3 exact tallies per range, {#signum(d) == y, #signum(d) == 0, #signum(d) == -y}.
 *   range_loss_out  (may be NULL) one double per range: the bits of dsgd_lg_loss_acc on range r alone (every range has its
 *                   own workgroups, the grid of a launch of its own, and its own words of partial sums); 0.0 for an empty
 *                   range.  counts_out[3 r] / rows of r is that call's accuracy.
 *   loss, acc       (either may be NULL) over all n rows: loss = lambda |w|^2 + (the ranges' sums of l_i, added in range
 *                   order) / n, acc = (the ranges' first tallies, added) / n; |w|^2 from the same per-workgroup words as
 *                   dsgd_lg_loss_acc.  The same call gives the same bits.
 * An empty range (begin == end) is an empty reply: no bytes, zero tallies.  DSGD_EINVAL, nothing written: a null ctx or
 * null ranges, n_ranges < 1 or > 256, begin > end, ranges that overlap, no rows at all, every output NULL.  Rows outside the
 * loaded data: DSGD_ERANGE, nothing written.
 *
 * dsgd_lg_loss_acc_list: loss and accuracy over the n >= 1 rows idx names, ONE launch.  A row named twice is counted twice.
 * loss = lambda |w|^2 + (sum of l_i) / n, acc = c0 / n, counts (3, may be NULL) the exact tallies as above; loss and acc may
 * be NULL.  For idx = b, b + 1, ..., e - 1 the figures are the bits of dsgd_lg_loss_acc(b, e); the same list gives the same
 * bits every time (a list in another order may differ in the last bits of the loss: the sum follows the list).
 * DSGD_EINVAL: a null ctx or idx, n < 1; DSGD_ERANGE: an entry outside the loaded rows; nothing written either way.
 *
 * dsgd_lg_loss_acc_sampled: dsgd_loss_acc_sampled for this model, word for word -- the same draw on the device from
 * *jstate (the first n = min(samples_count, len) entries of Random.shuffle(0 until len), entry p naming row row_begin + p),
 * the same *n_out / *draws_out / idx_out, the same limits (len up to 2^20 rows, at most 512 rejections inside the shuffle)
 * and beyond them the same DSGD_EUNSUPPORTED with nothing drawn, *jstate untouched and nothing written; len == 1 draws
 * nothing and evaluates that row.  Its figures are the bits of dsgd_lg_loss_acc_list on idx_out.  DSGD_EINVAL, nothing
 * written or drawn: a null ctx or jstate, samples_count < 1, row_begin >= row_end; a window outside the loaded rows:
 * DSGD_ERANGE.
 *
 * All three: w == NULL uses the resident weights, otherwise w replaces them (as in dsgd_lg_loss_acc).  The family's other
 * refusals hold (above): an fp64 context and a communicator of dsgd_comm_init / dsgd_comm_init_all DSGD_EUNSUPPORTED, no data
 * or a running lock-free engine DSGD_ESTATE.  Under dsgd_comm_init_lg they are LOCAL: no collective is entered, the figures
 * are the shard's.  They leave the weights, the accumulators and the cached |w|^2 words as dsgd_lg_loss_acc leaves them: a
 * step, a gradient or an evaluation behind them gives the bits it gives without them.
 *
 * ASYNCHRONOUS (the zero-lag schedule; csrc/dsgd_logistic.hpp, csrc/dsgd_lg_cs_async.hpp; ref: core/Slave.scala:79-111, 177-185,
 * core/MasterAsync.scala).  One update is ONE worker's, over a list of n >= 1 rows, on the resident fp32 weights: the int64
 * column sums of dsgd_lg_gradient's launch on S = lg_shift(n), then per column, fp64 with contraction off,
 *     G = acc 2^(vexp - S),  gm = G / n,  r = gm + 2 lambda w_j,  delta_j = lr r,  w_j' = (float)(w_j - delta_j)
 * -- the MEAN over the list (not over workers), regularised once, one rounding to float.  For n = 1 the weights are the bits
 * of dsgd_lg_sync_step with one worker on that row.  The delta is DENSE (plain L2 moves every column) and DOUBLE (the
 * reference's wire value); a peer applies w_k = (float)((double)w_k - dv_k), the same expression, so replicas that exchange
 * every delta stay bit-identical.  lr is a double throughout (the reference's learning rate is a Double).
 *   dsgd_lg_async_step     one update over idx[0 .. n); delta_out NULL or D + 1 doubles in key order; the statistics and the
 *                          |w'|^2 words as dsgd_lg_sync_step leaves them.  n < 1 or a null idx: DSGD_EINVAL
 *   dsgd_lg_update_grad    a peer's (key, dv) pairs.  The keys are checked on the host first: outside [0, D] DSGD_ERANGE, repeated
 *                          DSGD_EINVAL, the weights unchanged either way; nnz == 0 is a no-op.  The |w|^2 words are stale
 *                          afterwards, as for weights set by the caller
 *   dsgd_async_plan_create_lg, dsgd_async_plan_create_lg_cs   dsgd_async_plan_create's arguments on an fp32 context: updates
 *                          [first_update, first_update + n_updates) of the schedule -- update u is worker u mod K at its
 *                          iteration u div K -- as a ONE-worker logistic plan whose lists the device draws
 *                          (oracle/hogwild_replay.hog_rows restates them).  The row form takes any batch.  _lg_cs additionally
 *                          lays out the column slices; a batch beyond 1,024 rows or a model 16 slices cannot hold at one worker
 *                          is refused at creation (DSGD_EUNSUPPORTED, nothing drawn); COLUMN SLICES' softer declines leave the
 *                          row form (vals[0] = 7)
 *   dsgd_plan_run_async_lg the updates [step_begin, step_end) of ANY one-worker logistic plan, a caller's from
 *                          dsgd_plan_create_lg_n / _lg_cs_n included: two launches per update with no host synchronisation in
 *                          between (the bits of dsgd_lg_async_step on the same lists), or on current column slices ONE launch
 *                          of dsgd_lg_cs_async_kernel for the whole range -- COLUMN SLICES' layout, exchange, bounded wait
 *                          and numerics (deterministic, within tests/logistic_async_bound.py of the fp64 model, not the row
 *                          form's bits; no |w'|^2 words left).  dsgd_synchronize reports the rows.  dsgd_plan_run on these
 *                          plans keeps meaning the synchronous step
 *   refused                nothing enqueued, nothing changed: a plan of more than one worker DSGD_EINVAL; a plan that is not
 *                          logistic, an fp64 context, ANY communicator attached (dsgd_comm_init_lg's too: the schedule is one
 *                          process's) DSGD_EUNSUPPORTED; no data or a running lock-free engine DSGD_ESTATE
 *
 * SEVERAL TOPICS (csrc/dsgd_lg_topics.hpp).  One-vs-rest over T label planes on the SAME resident rows: the
 * rows, their ranking, vexp and the lists do not depend on the label, only c = -y / (1 + exp(y d)) and the weight vector do.
 * The planes and the topics' weights live beside the context's own labels and weights and touch neither: dsgd_get_weights,
 * dsgd_lg_loss_acc and every other entry point see what they saw before.  A step is TWO launches whatever T
 * (dsgd_lg_topics_grad_kernel: a row's first 64 non-zeros fetched once for all topics; dsgd_lg_topics_finish_kernel: one
 * column per lane, the topic on the grid's second dimension), an evaluation ONE (dsgd_lg_topics_eval_kernel).
 * THE CONTRACT: topic t's weights, losses, accuracies and probabilities are the BITS that dsgd_lg_sync_step / _sync_steps /
 * _loss_acc / _predict give on a context that holds the same rows with label = plane t, from the same weights, lists, lr and
 * lambda (the column sums are exact integers, so sharing the pass and the LDS head moves no bit; the tile rule above covers
 * the evaluation's smaller per-topic tile).
 *   dsgd_lg_topics_set          1 <= T <= 8 (LG_TOPICS_MAX) planes of n_rows entries each, topic-major, each +1 or -1; the
 *                               topics' weights start at zero.  T = 0 drops the topics and frees their memory.  Setting again
 *                               replaces planes and weights; an allocation failure leaves the context as it was
 *   dsgd_lg_topics_count        T as it is now (0: no topics) -- what sizes the arrays of the calls below
 *   dsgd_lg_topics_set_weights / _get_weights   T x (D + 1) floats, topic-major, key order
 *   dsgd_lg_topics_sync_step    dsgd_lg_sync_step's arguments: one step of every topic over the same K lists
 *   dsgd_lg_topics_sync_steps   dsgd_lg_sync_steps' arguments: 2 n_steps launches, no host synchronisation in between
 *   dsgd_lg_topics_loss_acc     loss[t], acc[t] over rows [row_begin, row_end) (either array may be NULL, not both)
 *   dsgd_lg_topics_predict      sigma(d_t) of every listed position: p_out[t * n + position]
 *   refused                     before anything is enqueued, nothing written: T outside [0, 8], a null pointer or a plane entry
 *                               other than +1/-1 DSGD_EINVAL; an index outside the data DSGD_ERANGE; an fp64 context or ANY
 *                               communicator attached (dsgd_comm_init_lg's too) DSGD_EUNSUPPORTED; no data, a running lock-free
 *                               engine, or no topics set DSGD_ESTATE.  dsgd_load_csr / _f64 drops the topics (the planes label
 *                               the rows that went), and so does a new column ranking (a communicator attached and detached):
 *                               the calls return DSGD_ESTATE until topics are set again (that drop comes BEHIND a call's
 *                               argument checks: a call refused for its arguments has changed nothing)
 *
 * LIMITS (out of scope, each refused or simply absent): several topics run per-call steps over lists only -- no plans, no
 * row ranges or column lists, no column slices, no ranks, no asynchronous iteration, one lambda and one lr for all topics,
 * no JNI; no JNI / Scala binding and nothing in include/dsgd.hpp; the host
 * mirrors are host.LogisticSync and host.LogisticAsync (Master.fit's and MasterAsync.fit's flow on one context, no
 * communicator -- host.LogisticSync(ranks=(world, rank)) additionally runs Master.fit across dsgd_comm_init_lg's ranks;
 * host.MasterSync / MasterAsync stay the SVM's); no fused or persistent one-launch step and no column
 * slices but those of COLUMN SLICES and ASYNCHRONOUS above; no asynchronous engine of the lock-free kind (dsgd_async_start
 * and dsgd_hogwild_kernel stay the SVM's: their parity rests on gate traces a gateless model does not have); no fp64 contexts
 * and no Double feature values; across ranks only what ACROSS RANKS lists -- no device-drawn lists but the job
 * form's (dsgd_plan_create_from_seed_job_lg), no column slices, no asynchronous iteration, no evaluation summed over the ranks
 * but dsgd_lg_eval_job's tallies and losses (classes and probabilities are a rank's own rows'; no sampled evaluation across
 * ranks: the sampled window is the master's data); no Sparse boundary forms.
 *
 * dsgd_lg_gradient: one worker's regularised sum over the listed rows, key order, from the resident weights or from w
 * (which then replaces them, as in dsgd_gradient).  dsgd_lg_sync_step / _ranges: one step over K lists / K row
 * ranges [row_begin[k], row_end[k]).  dsgd_lg_sync_steps: an epoch's steps in ONE call -- the lists are uploaded once,
 * two launches per step, no host synchronisation in between; offsets as in dsgd_sync_steps_f64 (n_steps * n_workers + 1
 * positions into idx, step-major, worker-minor).  dsgd_lg_loss_acc: the reported loss and the share of rows with
 * signum(d) == y over rows [row_begin, row_end); the same call gives the same bits (fixed-order sums).
 * dsgd_lg_predict: sigma(d) of every listed position, computed in fp64 from the fp32 d and rounded to float once.    */
int dsgd_lg_gradient(dsgd_ctx* ctx, const float* w /* NULL = resident */, const int32_t* idx, int64_t n, float* g_out /* D+1, key order */,
                     dsgd_batch_stats* stats);
int dsgd_lg_sync_step(dsgd_ctx* ctx, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers, float lr,
                      dsgd_batch_stats* stats);
int dsgd_lg_sync_step_ranges(dsgd_ctx* ctx, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, float lr,
                             dsgd_batch_stats* stats);
int dsgd_lg_sync_steps_ranges(dsgd_ctx* ctx, const int64_t* row_begin, const int64_t* row_end, int32_t n_workers, int64_t n_steps, float lr,
                              dsgd_batch_stats* stats);
int dsgd_lg_sync_steps(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets /* n_steps * n_workers + 1 */, int64_t n_steps,
                       int32_t n_workers, float lr, dsgd_batch_stats* stats);
int dsgd_lg_loss_acc(dsgd_ctx* ctx, const float* w /* NULL = resident */, int64_t row_begin, int64_t row_end, double* loss, double* acc);
int dsgd_lg_predict(dsgd_ctx* ctx, const float* w /* NULL = resident */, const int32_t* idx, int64_t n, float* p_out /* n */);
int dsgd_plan_create_lg_n(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets /* n_steps * n_workers + 1 */, int64_t n_steps,
                          int32_t n_workers, dsgd_plan** out);
int dsgd_plan_create_from_seed_lg(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end, int32_t n_splits,
                                  int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out);
int dsgd_plan_create_lg_cs_n(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets /* n_steps * n_workers + 1 */, int64_t n_steps,
                             int32_t n_workers, dsgd_plan** out);
int dsgd_plan_create_from_seed_lg_cs(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* split_begin, const int64_t* split_end, int32_t n_splits,
                                     int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out, int64_t* draws_out);
int dsgd_lg_loss_acc_ranges(dsgd_ctx* ctx, const float* w /* NULL = resident */, const int64_t* row_begin, const int64_t* row_end, int32_t n_ranges,
                            double* loss_out /* n_ranges */, double* acc_out /* n_ranges */);
int dsgd_lg_async_step(dsgd_ctx* ctx, const int32_t* idx, int64_t n, double lr, double* delta_out /* D+1, key order, or NULL */,
                       dsgd_batch_stats* stats);
int dsgd_lg_update_grad(dsgd_ctx* ctx, const int32_t* key, const double* dv, int64_t nnz);
int dsgd_async_plan_create_lg(dsgd_ctx* ctx, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers, int32_t batch,
                              uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates, dsgd_plan** out);
int dsgd_async_plan_create_lg_cs(dsgd_ctx* ctx, const int64_t* assigned_begin, const int64_t* assigned_end, int32_t n_workers, int32_t batch,
                                 uint64_t seed, int32_t positional_bug, int64_t first_update, int64_t n_updates, dsgd_plan** out);
int dsgd_plan_run_async_lg(dsgd_ctx* ctx, dsgd_plan* plan, int64_t step_begin, int64_t step_end, double lr);
int dsgd_lg_predict_ranges(dsgd_ctx* ctx, const float* w /* NULL = resident */, const int64_t* row_begin, const int64_t* row_end, int32_t n_ranges,
                           int8_t* class_out /* sum of lengths, may be NULL */, float* proba_out /* sum of lengths, may be NULL */,
                           int64_t* counts_out /* 3 * n_ranges or NULL */, double* range_loss_out /* n_ranges or NULL */,
                           double* loss /* may be NULL */, double* acc /* may be NULL */);
int dsgd_lg_loss_acc_list(dsgd_ctx* ctx, const float* w /* NULL = resident */, const int32_t* idx, int64_t n, double* loss, double* acc,
                          int64_t* counts /* 3 or NULL */);
int dsgd_lg_loss_acc_sampled(dsgd_ctx* ctx, const float* w /* NULL = resident */, uint64_t* jstate, int64_t row_begin, int64_t row_end,
                             int64_t samples_count, double* loss, double* acc, int64_t* counts /* 3 or NULL */,
                             int32_t* idx_out /* min(samples_count, row_end - row_begin) rows or NULL */, int64_t* n_out, int64_t* draws_out);
/* across ranks ("ACROSS RANKS" above): a rank's window of the job's device-drawn lists; the job's evaluation on every rank */
int dsgd_plan_create_from_seed_job_lg(dsgd_ctx* ctx, uint64_t* jstate, const int64_t* job_len, int32_t n_job, int32_t first, int32_t n_local,
                                      const int64_t* split_begin, int64_t max_samples, int32_t batch_size, dsgd_plan** out, int64_t* n_steps_out,
                                      int64_t* draws_out);
int dsgd_lg_eval_job(dsgd_ctx* ctx, const float* w /* NULL = resident */, const int64_t* row_begin, const int64_t* row_end, int32_t n_local,
                     int64_t* counts_out /* 3 * K or NULL */, double* range_loss_out /* K or NULL */, double* loss /* may be NULL */,
                     double* acc /* may be NULL */, int32_t* K_out /* may be NULL */);
/* several topics ("SEVERAL TOPICS" above) */
int dsgd_lg_topics_set(dsgd_ctx* ctx, int32_t T, const int8_t* planes /* T x n_rows, topic-major, each +1 or -1 */);
int dsgd_lg_topics_count(dsgd_ctx* ctx, int32_t* T_out /* the topics set now; 0: none */);
int dsgd_lg_topics_set_weights(dsgd_ctx* ctx, const float* W /* T x (D+1), key order */);
int dsgd_lg_topics_get_weights(dsgd_ctx* ctx, float* W_out /* T x (D+1), key order */);
int dsgd_lg_topics_sync_step(dsgd_ctx* ctx, const int32_t* const* idx_per_worker, const int64_t* n_per_worker, int32_t n_workers, float lr,
                             dsgd_batch_stats* stats);
int dsgd_lg_topics_sync_steps(dsgd_ctx* ctx, const int32_t* idx, int64_t n_idx, const int64_t* offsets /* n_steps * n_workers + 1 */,
                              int64_t n_steps, int32_t n_workers, float lr, dsgd_batch_stats* stats);
int dsgd_lg_topics_loss_acc(dsgd_ctx* ctx, int64_t row_begin, int64_t row_end, double* loss /* T */, double* acc /* T */);
int dsgd_lg_topics_predict(dsgd_ctx* ctx, const int32_t* idx, int64_t n, float* p_out /* T x n, topic-major */);

#ifdef __cplusplus
}
#endif
#endif /* DSGD_H */
