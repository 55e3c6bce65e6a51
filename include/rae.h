/*
 * rae.h -- C ABI of the MI355X-native relation-autoencoder training path.
 *
 * This is the drop-in boundary for the reference's compiled Theano function
 *
 *   self.func['train'] = theano.function(inputs=[batch_index, neg1, neg2], outputs=cost,
 *                                        updates=..., givens={xFeats, ents_1, ents_2})
 *        (learning/OieInduction.py:146-149, called at :189)
 *   self.func['label_<split>'] = theano.function(inputs=[batch_index],
 *                                        outputs=(labels, probs), ...)
 *        (learning/OieInduction.py:151-155, called at :245,259,337)
 *
 * and for the model/optimizer objects that function is built from
 * (OieModelFunctions learning/OieModel.py:16-101, AdaGrad/SGD learning/Optimizers.py:6-52).
 *
 * Conventions
 *  - plain C types only; every pointer named *_dev is a device pointer (HBM, gfx950);
 *  - the caller owns all parameter / accumulator / data / exchange memory (they are
 *    Theano shared variables in the reference: learning/OieInduction.py:439-449,
 *    learning/Optimizers.py:12-15); the plan holds borrowed pointers plus a private
 *    workspace allocated once in rae_plan_create;
 *  - every call returns 0 on success and a negative RAE_E* code on error;
 *    rae_last_error() returns a thread-local message for the last failure;
 *  - hot calls (rae_step_*, rae_train_step, rae_label) never allocate or synchronise, so
 *    they can be captured into a HIP graph; they are stream-ordered on `stream`;
 *  - a plan is single-caller (like a Theano function); different plans may run on
 *    different streams concurrently.
 */
#ifndef RAE_H
#define RAE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* rae_stream_t;   /* == hipStream_t */

#define RAE_OK 0
#define RAE_E_INVALID (-1)     /* bad argument / unsupported configuration           */
#define RAE_E_HIP (-2)         /* HIP runtime error                                  */
#define RAE_E_OVERFLOW (-3)    /* a per-step row-index partition overflowed its LDS  */
#define RAE_E_STATE (-4)       /* call sequence error; a peer-to-peer wait timed out */
/* device error word bits (rae_check; rae_last_error names each set bit): 1 / 2 an A / W
 * row-index partition overflowed its LDS sort, 4 a batch exceeded the index's record capacity,
 * 8 a data-parallel row list overflowed while being built, 16 a row list is longer than the
 * exchange's row capacity (RAE_E_OVERFLOW for these); 64 a peer-to-peer wait timed out -- a
 * peer stopped signalling (RAE_E_STATE)                                                      */

/* decoder type: learning/models/decoders/Decoder.py:84-93 ('sp', 'rescal', 'rescal+sp') */
#define RAE_DEC_SP 0
#define RAE_DEC_RESCAL 1
#define RAE_DEC_HYBRID 2

/* optimizer: learning/OieInduction.py:261-269 ('adagrad', 'sgd') */
#define RAE_OPT_ADAGRAD 0
#define RAE_OPT_SGD 1

/* negative-sample column addressing */
#define RAE_NEG_PER_CALL 0     /* neg arrays are (s, l_global): column = example-in-batch */
#define RAE_NEG_PER_EPOCH 1    /* neg arrays are (s, N): column = global example index     */

typedef struct rae_config {
    int32_t decoder;          /* RAE_DEC_*                                                */
    int32_t optimizer;        /* RAE_OPT_*                                                */
    int64_t n_examples;       /* N: rows of the train split (learning/OieData.py:78)     */
    int64_t n_features;       /* d: feature dimensionality (OieData.py:96-98)             */
    int64_t n_entities;       /* n: entity vocabulary (OieData.py:92-94)                  */
    int32_t relations;        /* m = K (--relations, OieInduction.py:469)                 */
    int32_t embed;            /* r (--embed-size, :468)                                   */
    int32_t neg_samples;      /* s (--neg-samples, :470)                                  */
    int32_t batch_size;       /* l: examples per rank per step (--batch-size, :467)       */
    int32_t world_size;       /* data-parallel ranks G (1 = single GPU)                   */
    int32_t rank;             /* this rank                                                */
    float learning_rate;      /* --learning-rate (:466)                                   */
    float alpha;              /* entropy scale (--alpha, :479; OieModel.py:81)            */
    float lambda1;            /* --l1 (:471)                                              */
    float lambda2;            /* --l2 (:472)                                              */
    int32_t ext_reg;          /* --ext-reg (:477; OieModel.py:60-62)                      */
    int32_t max_batch_nnz;    /* max nnz over global batches (sizes the W row index)      */
    int32_t max_row_nnz;      /* max nnz of one example row                               */
    int32_t neg_mode;         /* RAE_NEG_*                                                */
    int64_t neg_stride;       /* row stride (elements) of the neg arrays                  */
    int64_t index_window;     /* batches whose row index is held at once (0 = default)   */
    int32_t mfma_bf16;        /* RESCAL / hybrid: bf16 MFMA operands for the R/C GEMMs    *
                               * (fp32 accumulate; BASELINE config 5); 0 = exact fp32     */
    /* kernel forms (0 = the plan's own choice for the shape; the others exist so tests can
     * pin one form against another -- every form computes the same step):                 */
    int32_t sp_forward;       /* SP forward: RAE_SPFWD_*                                    */
    int32_t bil_dp;           /* bilinear dCost/dP contraction: RAE_BILDP_*                 */
    int32_t bil_prep;         /* bf16 R-gradient operands: RAE_BILPREP_*                    */
    int32_t dp_update;        /* data-parallel update: RAE_DPUPD_*                          */
    int32_t priv_rows;        /* rows one record of the batch references: RAE_PRIV_*        */
    int32_t dp_dense;         /* data-parallel SP: dense decoder-matrix gradients RAE_DPDENSE_* */
    int32_t heavy_chunk;      /* very heavy rows split into record chunks: RAE_HCHUNK_*      */
    int32_t dp_xchg;          /* data-parallel exchange: RAE_XCHG_*                          */
} rae_config;

#define RAE_SPFWD_AUTO 0      /* fused per-example kernel unless r*m > 32768                  */
#define RAE_SPFWD_FUSED 1     /* k_forward: one workgroup per example                         */
#define RAE_SPFWD_SPLIT 2     /* k_sp_enc -> P.C^T GEMM -> k_sp_dec -> dw.C GEMM (+ dS epilogue)  */
#define RAE_BILDP_AUTO 0      /* inside the second M-tile pass when bf16 and m <= 128          */
#define RAE_BILDP_STRIDED 1   /* k_bil_dp (one wave per 16x16 tile of dP)                      */
#define RAE_BILDP_STAGED 2    /* k_bil_dp2 (bf16, LDS-staged R slices; r <= 256, m <= 128)      */
#define RAE_BILDP_MTILE 3     /* inside the second k_bil_mt pass (bf16, m <= 128)               */
#define RAE_BILPREP_AUTO 0    /* single rank: the forward writes the operands (no launch)      */
#define RAE_BILPREP_KERNEL 1  /* k_bil_prep after the exchange                                 */
#define RAE_DPUPD_REPLICATED 0 /* every rank updates every referenced row (bit-identical     *
                                * replicas after every step)                                  */
#define RAE_DPUPD_PARTITIONED 1 /* rank k updates the rows it owns (row % G == k) and pushes *
                                 * the next step's rows to the ranks that read them            */
#define RAE_PRIV_AUTO 0       /* rows exactly one record of the global batch references are left  *
                               * out of the update's row tasks and updated by per-example        *
                               * workgroups of the same update launch (task_private_rows; the    *
                               * one-record row task's arithmetic, bit-identical parameters) in  *
                               * single-rank and replicated plans with a global batch below 4096 *
                               * examples, without a regulariser (lambda1 = lambda2 = 0) and     *
                               * with 2 + 2s <= 64 record slots, any decoder                     */
#define RAE_PRIV_OFF 1        /* every row updated by the update's row tasks                      */
#define RAE_PRIV_ON 2         /* private rows whenever admissible (no regulariser, <= 64 slots),   *
                               * any global batch; the partitioned update takes the private rows *
                               * it owns, one wave per example                                    */
#define RAE_DPDENSE_AUTO 0    /* partials when they are at most half of dw1 / dw2 in the records *
                               * (per-rank partial chunk <= r floats: l >~ 2 relations)          */
#define RAE_DPDENSE_RECORDS 1 /* dw1 / dw2 of every example in the exchange records; the update *
                               * reduces dC1 / dC2 / dWb over the global batch (K = L)           */
#define RAE_DPDENSE_PARTIALS 2 /* each rank reduces its own l examples' dC1 / dC2 / dWb before   *
                                * the exchange (k_dpart); the records carry the partial block,  *
                                * the update sums the ranks' blocks in rank order               */
#define RAE_HCHUNK_AUTO 0     /* global batches of >= 2048 examples: rows with at least 256      *
                               * records of the batch summed as floor(records / 128) chunks in   *
                               * parallel (128 records each, the last one to the row's end; one  *
                               * partial per chunk, k_heavy_fin adds them in chunk order and     *
                               * applies the optimiser); smaller batches: off                    */
#define RAE_HCHUNK_OFF 1      /* every very heavy row summed by one workgroup                      */
#define RAE_HCHUNK_ON 2       /* chunks at any global batch                                        */
#define RAE_XCHG_COLLECTIVE 0 /* the caller moves records / rows between the step launches (an    *
                               * all-gather; rae_dp_pack -> all-to-all -> rae_dp_unpack)         */
#define RAE_XCHG_P2P 1        /* partitioned update only: the kernels store records and rows     *
                               * straight into the peers' buffers (rae_set_peer) and wait on     *
                               * their signal counters -- no caller collective in the step       */
#define RAE_XCHG_P2P_PIPE 2   /* RAE_XCHG_P2P with the next batch's rows pushed during this step: *
                               * the rows the update leaves unchanged right after the forward,   *
                               * every updated row by the update task that writes it -- so the   *
                               * row bytes travel under the update; world_size <= 8, private     *
                               * rows off; rae_p2p_prologue before the first step of a run       */

/* Caller-owned device buffers.  Shapes are the reference's (fp32 everywhere):
 *   W (d,m)  Wb (m)  A (n,r)  Ab (n)  C1,C2 (r,m)  R (r,r,m) [rescal] / C (r,r,m) [hybrid]
 *   (RelationClassifier.py:24-25, OieModel.py:105, SelectionalPreferences.py:13-19,
 *    Bilinear.py:14-17, BilinearPlusSP.py:14-23), acc_* the AdaGrad accumulators of the
 *   same shapes (Optimizers.py:12-15; unused for SGD, may be NULL).
 * data: the train split CSR (OieData.py:83-90) + entity ids.  values may be NULL
 *   (binary features: every stored value is 1.0, OieData.py:88).
 * exchange: per-example records of the global batch, rae_exchange_floats() floats; rank k
 *   writes rows [k*l, (k+1)*l); between rae_step_forward and rae_step_update the caller
 *   all-gathers it across ranks (no-op for world_size == 1).
 * costs: one float per batch index (the value func['train'] returns).
 */
typedef struct rae_buffers {
    float* W; float* Wb; float* A; float* Ab;
    float* C1; float* C2; float* R3;             /* R3 = R (rescal) or C (hybrid) */
    float* acc_W; float* acc_Wb; float* acc_A; float* acc_Ab;
    float* acc_C1; float* acc_C2; float* acc_R3;
    const int32_t* indptr; const int32_t* indices; const float* values;
    const int32_t* args1; const int32_t* args2;
    const int32_t* neg1; const int32_t* neg2;   /* may be NULL until rae_set_negatives */
    float* exchange;
    float* costs;
} rae_buffers;

typedef struct rae_plan rae_plan;

/* --- lifetime ---------------------------------------------------------------------- */
int rae_plan_create(const rae_config* cfg, const rae_buffers* buf, rae_plan** out);
int rae_plan_destroy(rae_plan* plan);
const char* rae_last_error(void);
int rae_version(void);
/* hash of the sources and flags the library was built from (rae/_lib.py source_build_id);
 * the Python binding refuses a library whose id differs from the sources beside it       */
const char* rae_build_id(void);

/* floats per example record and per global batch in the exchange buffer.  A plan needs
 * rae_exchange_floats() < 2^30 (4 GiB; rae_plan_create returns RAE_E_INVALID otherwise): the
 * update reads a record through a buffer resource at a 32-bit byte offset from the buffer's
 * base, so records at or beyond 2^30 floats cannot be addressed.                          */
int64_t rae_exchange_record_floats(const rae_config* cfg);
int64_t rae_exchange_floats(const rae_config* cfg);

/* The kernel forms the plan resolved for its shape (RAE_SPFWD_FUSED / _SPLIT, RAE_BILDP_*,
 * RAE_BILPREP_*, RAE_DPUPD_*, RAE_PRIV_*; 0 where a form does not apply to the decoder), written into
 * the matching fields of *out (the other fields are left as they are).                  */
int rae_plan_forms(const rae_plan* plan, rae_config* out);

/* --- negatives --------------------------------------------------------------------- */
/* Point the plan at negative-sample arrays (learning/NegativeExampleGenerator.py:14-32
 * output, int32).  mode RAE_NEG_PER_EPOCH: (s, N) arrays for the whole epoch
 * (OieInduction.py:183-184); RAE_NEG_PER_CALL: (s, l_global) arrays of one batch
 * (OieInduction.py:187-189). */
int rae_set_negatives(rae_plan* plan, const int32_t* neg1_dev, const int32_t* neg2_dev,
                      int32_t mode, int64_t stride);

/* --- the row index ----------------------------------------------------------------- */
/* Build the per-batch row index (for every parameter row a batch references, its
 * contributing records in a fixed order) for global batches [first, first+count), from the
 * current negatives; count <= rae_index_window().  Batch b uses slot b % window, so build
 * a window before stepping through it.  Independent of the parameters. */
int rae_build_index(rae_plan* plan, int64_t first_batch, int64_t count, rae_stream_t stream);
int64_t rae_index_window(rae_plan* plan);

/* Read-back of the row index (tests and diagnosis; read-only, outside every step path).
 * The index dimensions the plan resolved, as RAE_INDEX_NDIMS int64 values in this order:
 * L, l, s, G, rank, part, RA, RW, HA, HW, index_window, posbits, TC, NVC, hch, HF, dcap,
 * dstride, dnx, priv, privnf, LA, LW  (RA / RW: record slots per batch and table; TC / NVC /
 * HF: entries per slot of task / vtask / hfin; LA / LW: row-list capacities).  count must be
 * RAE_INDEX_NDIMS.                                                                          */
#define RAE_INDEX_NDIMS 23
int rae_index_dims(const rae_plan* plan, int64_t* out, int32_t count);
/* Regions of a batch slot (slot = batch % index_window), 32-bit ints throughout:
 *   SREC_A / _W   RA / RW record ids, sorted by (row, record), partition after partition
 *   SEG_A / _W    RA / RW x 4: (row, first position, end position, first record id)
 *   COUNT_A / _W  1024 partition counts;  PCLS_A / _W  1024 x 4: (heavy, light, very heavy, offset)
 *   THDR          4: (wave tasks, workgroup tasks, chunked rows, 0)
 *   TASK          TC x 4;  VTASK  NVC x 4;  HFIN  HF x 4 (plans that chunk very heavy rows)
 *   DESC          dnx x dstride;  PMASK  L x 4 (plans with private rows)
 *   DPL           2 x G x (LA + LW) row lists, DPC 2 x G x 2 their lengths [dir][peer][table],
 *   DPMAX         2: the longest entity / feature list since the last rae_dp_list_max (not per
 *                 slot)  (these three: the partitioned update only)
 * Entries behind what the counts cover are stale by design.                                 */
#define RAE_IDXR_SREC_A 0
#define RAE_IDXR_SREC_W 1
#define RAE_IDXR_SEG_A 2
#define RAE_IDXR_SEG_W 3
#define RAE_IDXR_COUNT_A 4
#define RAE_IDXR_COUNT_W 5
#define RAE_IDXR_PCLS_A 6
#define RAE_IDXR_PCLS_W 7
#define RAE_IDXR_THDR 8
#define RAE_IDXR_TASK 9
#define RAE_IDXR_VTASK 10
#define RAE_IDXR_HFIN 11
#define RAE_IDXR_DESC 12
#define RAE_IDXR_PMASK 13
#define RAE_IDXR_DPL 14
#define RAE_IDXR_DPC 15
#define RAE_IDXR_DPMAX 16
/* Synchronises the device, then copies the region of `batch`'s slot to host memory.  bytes
 * must be the region's size; RAE_E_INVALID for a wrong size or a region the plan does not
 * have (HFIN without chunks, PMASK without private rows, DPL / DPC / DPMAX outside the
 * partitioned update).                                                                      */
int rae_index_read(rae_plan* plan, int64_t batch, int32_t region, void* host_out, int64_t bytes);

/* --- the training step (func['train']) --------------------------------------------- */
/* Batch addressed as  batch = *cursor + step_offset  (cursor: device int64 owned by the
 * plan) so a captured sequence of steps can be replayed for successive batches.        */
int rae_set_cursor(rae_plan* plan, int64_t batch, rae_stream_t stream);
int rae_advance_cursor(rae_plan* plan, int64_t count, rae_stream_t stream);
/* Number of rae_set_cursor / rae_advance_cursor calls made on this plan so far (host count;
 * a captured graph's replays make no calls).  A driver that caches where the cursor points
 * compares it with the count it saw last, so a move made by anyone else is never missed.  */
int64_t rae_cursor_moves(const rae_plan* plan);
/* K1: per-example encoder + decoder forward/backward of this rank's l examples.  Writes the
 * exchange records.  The batch's row index must have been built (rae_build_index).      */
int rae_step_forward(rae_plan* plan, int64_t step_offset, rae_stream_t stream);
/* K2 (+K3 when lambda1/lambda2 != 0): deterministic per-row gradient reduction over the
 * global batch and the optimizer update of every parameter; writes costs[batch].        */
int rae_step_update(rae_plan* plan, int64_t step_offset, rae_stream_t stream);
/* The same two phases for an absolute global batch index (no device cursor: the index is a
 * launch argument; rae_train_step runs this way).  Measured on MI355X: no faster than the
 * cursor form inside graphs (the cursor load overlaps the kernels' other start-up loads),
 * and per-chunk graphs cost more to replay than one graph replayed over an epoch window.
 * `batch` in [0, n_examples / (batch_size * world_size)).                                */
int rae_step_forward_at(rae_plan* plan, int64_t batch, rae_stream_t stream);
int rae_step_update_at(rae_plan* plan, int64_t batch, rae_stream_t stream);
/* One whole func['train'](batch_index, neg1, neg2) call on a single rank:
 * rae_set_negatives(PER_CALL) + index + forward + update for `batch_index`.            */
int rae_train_step(rae_plan* plan, int64_t batch_index, const int32_t* neg1_dev,
                   const int32_t* neg2_dev, rae_stream_t stream);
/* --- partitioned data-parallel update (dp_update = RAE_DPUPD_PARTITIONED) ------------- *
 * Row r of A / Ab / W is owned by rank r % world_size; rae_step_update updates the owned rows
 * only (the dense C1 / C2 / Wb / R / C stay replicated).  Before each step's forward every
 * rank refreshes the non-owned rows its examples read:
 *     rae_dp_pack -> [caller: all-to-all of world_size equal blocks, send -> recv] -> rae_dp_unpack
 * (the same cursor / absolute batch addressing as rae_step_forward / _at).  The peers' row lists
 * are built with the row index (rae_build_index).  Parameters equal the replicated form's
 * bitwise once the owners' rows are gathered (the caller's sync; rae/dist.py sync_rows).
 * Requires lambda1 = lambda2 = 0.                                                          */
/* floats of one peer block for the given row capacities (entity rows, feature rows)      */
int64_t rae_dp_block_floats(const rae_config* cfg, int32_t cap_entities, int32_t cap_features);
/* caller-owned send / recv buffers of world_size blocks each, and their row capacities;
 * every list the plan builds must fit (rae_dp_list_max; a longer one sets error flag 16)   */
int rae_set_dp_buffers(rae_plan* plan, float* send_dev, float* recv_dev, int32_t cap_entities,
                       int32_t cap_features);
/* longest list built since the previous call (synchronises; resets the maxima)           */
int rae_dp_list_max(rae_plan* plan, int32_t* max_entities, int32_t* max_features);
int rae_dp_pack(rae_plan* plan, int64_t step_offset, rae_stream_t stream);
int rae_dp_unpack(rae_plan* plan, int64_t step_offset, rae_stream_t stream);
int rae_dp_pack_at(rae_plan* plan, int64_t batch, rae_stream_t stream);
int rae_dp_unpack_at(rae_plan* plan, int64_t batch, rae_stream_t stream);

/* --- peer-to-peer exchange (dp_xchg = RAE_XCHG_P2P) ---------------------------------- *
 * Every rank maps its peers' exchange buffer, W, A, Ab and signal words (IPC handles, traded
 * once through the caller's process group) and hands them to its plan; rae_step_forward then
 * pushes the owned rows each peer's examples read into that peer's replica, waits for the
 * peers' rows, runs the forward and pushes its records into every peer's exchange buffer;
 * rae_step_update waits for the peers' records.  Graph-capturable (kernels only).  The row
 * capacities come from rae_set_dp_buffers(plan, NULL, NULL, caps) as in the collective form.
 * Replaces (learning/OieInduction.py:186-189 runs one process): the all-gather / all-to-all. */
#define RAE_IPC_HANDLE_BYTES 64
/* handle of the allocation holding dev_ptr, and dev_ptr's offset in it                     */
int rae_ipc_export(const void* dev_ptr, void* handle_out, int64_t* offset_out);
/* map another process's allocation (its base address; add the exported offset)            */
int rae_ipc_open(const void* handle, void** base_out);
int rae_ipc_close(void* base);
/* the plan's signal counters (device, uncached; export them to the peers)                  */
void* rae_p2p_signals(rae_plan* plan);
/* peer `peer`'s buffers as this process maps them                                          */
int rae_set_peer(rae_plan* plan, int32_t peer, float* exchange_dev, float* W_dev, float* A_dev,
                 float* Ab_dev, void* signals_dev);
/* how long one wait kernel may spin for a peer's signal before it sets error bit 64 and
 * gives up (default 5 s; a driver that does host work between steps -- per-batch evaluation
 * -- raises it or puts a host barrier in front of the next step)                          */
int rae_set_p2p_timeout(rae_plan* plan, double seconds);
/* RAE_XCHG_P2P_PIPE: each step pushes (and signals) the rows of the NEXT batch, so the first
 * step of a run needs its own batch's rows pushed first: marks and pushes the rows of
 * `batch` and signals them (every rank calls it with the same batch).  drain != 0: the step
 * before this run pushed rows for another batch -- consume that signal first.  The row index
 * (rae_build_index) of a step's batch + 1 must be built before the step runs.            */
int rae_p2p_prologue(rae_plan* plan, int64_t batch, int32_t drain, rae_stream_t stream);

/* Kernel timing (bench / profiling; no reference counterpart).  Arms the NEXT
 * rae_step_forward or rae_step_update call on this plan: its kernels are launched with
 * hipExtLaunchKernelGGL so `start_event` takes the first kernel's dispatch-begin timestamp
 * and `stop_event` the last kernel's end timestamp -- the execution span rocprofv3
 * --kernel-trace reports, without event-packet overhead.  Not for graph capture.
 * Events are hipEvent_t handles (rae_event_create makes them).                         */
int rae_time_next(rae_plan* plan, void* start_event, void* stop_event);
int rae_event_create(void** event_out);
int rae_event_destroy(void* event);
/* waits for stop_event, then *ms = hipEventElapsedTime(start_event, stop_event) */
int rae_event_elapsed_ms(void* start_event, void* stop_event, float* ms);
/* Device error word (overflow flags); host reads it with rae_check() (a blocking read: waits
 * for all the device's queued work) or rae_check_on() (ordered on `stream` only: waits for
 * the work queued on that stream, e.g. a row-index build on a side stream).              */
int rae_check(rae_plan* plan);
int rae_check_on(rae_plan* plan, rae_stream_t stream);

/* --- negative sampling (learning/NegativeExampleGenerator.py:14-32) ----------------- */
/* out[i] = first j with cum[j] >= x_i  (numpy searchsorted side='left' over the float64 CDF
 * negSamplingCum, learning/OieData.py:57-59), i < count, int32.
 * rae_neg_sample:        x_i = uniforms[i], the caller's draws of U(0, cum[n-1]) -- with the
 *                        model's RandomState stream this is the reference sampler bit for bit.
 * rae_neg_sample_philox: x_i = cum[n-1] * U_i, U_i from Philox4x32-10 at counter offset + i
 *                        under key seed (device-only perf mode, not the reference's stream). */
int rae_neg_sample(const double* cum_dev, int64_t n, const double* uniforms_dev, int64_t count,
                   int32_t* out_dev, rae_stream_t stream);
int rae_neg_sample_philox(const double* cum_dev, int64_t n, uint64_t seed, uint64_t offset,
                          int64_t count, int32_t* out_dev, rae_stream_t stream);

/* --- labelling (func['label_<split>'], RelationClassifier.py:39-48) ----------------- */
/* rows [row0, row0+nrows) of any CSR split with the current W/Wb: labels = argmax(S)
 * (int64, first max) and probs = softmax(S) (fp32, may be NULL).                        */
int rae_label(const int32_t* indptr, const int32_t* indices, const float* values,
              const float* W, const float* Wb, int32_t relations, int64_t row0,
              int64_t nrows, int64_t* labels_out, float* probs_out, rae_stream_t stream);

/* --- forward-only objective (no reference counterpart: the reference's Theano function fuses
 * the update, learning/OieInduction.py:146-149) ------------------------------------------- */
/* The data term of the objective over rows [row0, row0+nrows) of any CSR split at the current
 * parameters, for 'sp', 'rescal' and 'rescal+sp'.  Plan-free like rae_label; every pointer is a
 * device pointer except the struct itself.  Per example b the reference's all_scores grouped by
 * example (learning/OieModel.py:80-90, the decoders' get_scores):
 *     terms[b] = (pos_b, H_b, neg_b)
 *     pos_b = logsig(u_b) + logsig(u_{l+b})        H_b = alpha * (-sum_k P log P)
 *     neg_b = sum over the example's 2s negative scores g of logsig(-g)
 * sums_out = the three column sums (S_pos, S_H, S_neg) in double; the data term of the cost is
 *     -(S_pos + 2 S_H + S_neg) / (nrows * (4 + 2s))
 * (the reference's denominator is l(4+2s), so this is the mean of the per-batch costs at any
 * batch size).  The L1 / L2 regularisers are NOT included.  SP keeps the reference's
 * A[args1]-twice behaviour (SelectionalPreferences.py:34-35); the hybrid uses A[args2].  Exact
 * fp32 (v_mfma_f32_16x16x4_f32) whatever operands training ran with.
 * An example's three terms are bitwise independent of row0, nrows and the other rows of the
 * call; sums_out depends only on the term values and nrows (one partial per 1024 rows, added in
 * row order, double).
 * The call allocates nothing, never synchronises and is stream-ordered (capturable); it writes
 * only terms_out, sums_out and workspace.  Arguments are checked before the first HIP call.
 * nrows == 0 is valid (zero sums).  Shapes: relations <= 512 (a multiple of 4 above 128; <= 320
 * for the bilinear decoders), embed <= 1024, at most 160 KiB of LDS per 16-example tile;
 * W / C1 / C2 / R3 16-byte aligned when relations % 4 == 0, A when embed % 4 == 0.            */
typedef struct rae_eval_args {
    int32_t decoder;            /* RAE_DEC_*                                                 */
    int32_t relations, embed, neg_samples;          /* m, r, s                               */
    int64_t n_entities;
    float   alpha;
    const float *W, *Wb, *A, *Ab, *C1, *C2, *R3;    /* unused ones may be NULL               */
    const int32_t *indptr, *indices; const float *values;   /* values may be NULL (binary)  */
    const int32_t *args1, *args2;
    const int32_t *neg1, *neg2; int64_t neg_stride; /* (s, >= row0+nrows): column = row index
                                                       within the split                      */
    int64_t row0, nrows;
    float  *terms_out;          /* (nrows, 3) fp32, may be NULL                              */
    double *sums_out;           /* 3 doubles                                                 */
    void   *workspace; int64_t workspace_bytes;
} rae_eval_args;
/* bytes of workspace rae_eval_cost needs for these arguments (host only, no HIP call; -1 on a
 * bad argument).  Independent of nrows: long ranges are processed in chunks.               */
int64_t rae_eval_workspace_bytes(const rae_eval_args* a);
int rae_eval_cost(const rae_eval_args* a, rae_stream_t stream);

/* --- argument ranking over the whole entity vocabulary (no reference counterpart: the reference
 * only scores s sampled negatives) ------------------------------------------------------------ */
/* rae_rank_queries: nq queries against all n_entities rows of A.  The score of entity e for query
 * q is  g_q(e) = <Q[q, :embed], A[e]> + (add[q] + Ab[e])  (add / Ab NULL: zero), one k-ascending
 * fp32 fmaf chain on v_mfma_f32_32x32x2_f32 (no split-K), never written to memory.  Outputs, over
 * the entities e in [0, n_entities) other than skip[q] (skip NULL or outside [0, n): nothing is
 * skipped):
 *     greater[q] = #{e : g_q(e) > target[q]}      equal[q] = #{e : g_q(e) == target[q]}
 *     lse[q] = log sum_e exp g_q(e)  (-inf when nothing is summed; lse may be NULL)
 * A query's three outputs are bitwise independent of nq, of its position and of the other
 * queries; the log-sum-exp is folded per entity strip (a count fixed by n_entities alone, at most
 * 128) and the strips are merged in order.  Every pointer is a device pointer except the struct.
 * Plan-free, stream-ordered, capturable: allocates nothing, never synchronises, writes only
 * greater, equal, lse and workspace; arguments are checked before the first HIP call.
 * Limits: nq >= 0 (0 is valid), 1 <= n_entities < 2^31, 1 <= embed <= 1024, ldq >= embed,
 * ldq % 4 == 0, Q 16-byte aligned, A 16-byte aligned when embed % 4 == 0, workspace 256-byte
 * aligned.  With nq == 0 no pointer is read.  Long query lists run in chunks of 4096.         */
typedef struct rae_rank_args {
    const float *Q; int64_t ldq; int64_t nq;
    const float *add;           /* (nq), may be NULL                                           */
    const float *target;        /* (nq)                                                        */
    const int32_t *skip;        /* (nq), may be NULL                                           */
    const float *A, *Ab;        /* (n_entities, embed), (n_entities) or NULL                   */
    int64_t n_entities; int32_t embed;
    int32_t *greater, *equal;   /* (nq)                                                        */
    float *lse;                 /* (nq), may be NULL                                           */
    void *workspace; int64_t workspace_bytes;
} rae_rank_args;
int rae_rank_queries(const rae_rank_args* a, rae_stream_t stream);

/* rae_eval_rank: both arguments of rows [row0, row0+nrows) of a split ranked against all
 * entities at the current parameters, with rae_eval_cost's scores.  P = softmax(x W + Wb),
 * a1 = A[args1], a2 = A[args2], M = sum_k P_k R3[:,:,k]:
 *     decoder     q1 (replaces arg 1)   q2 (replaces arg 2)   c1          c2          one
 *     sp          C1 P                  C2 P                  <C2 P,a1>   <C1 P,a1>   c1 + c2
 *     rescal      M a2                  M^T a1                0           0           <a1,q1>
 *     rescal+sp   M a2 + C1 P           M^T a1 + C2 P         <C2 P,a2>   <C1 P,a1>   <a1,q1> + c1
 * Query 2b + t - 1 (row b, side t): candidates g_t(e) = <A[e], q_t> + (c_t + Ab[e]), target
 * u_t = one + Ab[args_t] (the objective's positive score; SP keeps the reference's A[args1]-twice
 * behaviour, so u_2 != g_2(args2)), the true entity args_t left out.  Outputs as
 * rae_rank_queries', (nrows, 2).  Derived in double: rank = 1 + greater + equal / 2,
 * logp = u - logaddexp(u, lse);  summary[8 side + j], side = t - 1:
 *     j = 0 sum 1/rank   1 sum rank   2 sum logp   3..6 #{rank <= hits_k[j - 3]}   7 nrows
 * summed like rae_eval_cost's sums (one partial per 1024 rows, added in row order).
 * Reads decoder, shapes, parameters, CSR, args1 / args2, row0 / nrows and the workspace of `a`;
 * neg_samples, neg1, neg2, neg_stride, terms_out and sums_out are not read.  Shape limits are
 * rae_eval_cost's; rows run in chunks of 2048.  Plan-free, stream-ordered, capturable; writes
 * only the outputs and the workspace; per-query outputs are bitwise independent of row0, nrows
 * and the other rows.  nrows == 0 is valid (a zero summary).                                    */
typedef struct rae_rank_out {
    int32_t *greater, *equal;   /* (nrows, 2); not read when nrows == 0                        */
    float *target, *lse;        /* (nrows, 2), each may be NULL                                */
    double *summary;            /* 16 doubles, may be NULL                                     */
    int32_t hits_k[4];          /* <= 0: unused                                                */
} rae_rank_out;
int rae_eval_rank(const rae_eval_args* a, const rae_rank_out* out, rae_stream_t stream);

/* bytes of workspace of rae_rank_queries (q, with e NULL) or of rae_eval_rank (e, with q NULL);
 * host only, no HIP call; -1 on a bad argument or unless exactly one is given.  Reads the shapes
 * only; independent of nq / nrows; depends on n_entities only through the strip count (<= 128). */
int64_t rae_rank_workspace_bytes(const rae_rank_args* q, const rae_eval_args* e);

/* --- top-k entity retrieval: argument prediction and the selectional preferences of an induced
 * relation (no reference counterpart) ---------------------------------------------------------- */
/* rae_topk_queries: the `top` best-scoring entities of each of nq queries, with their scores.
 * The score g_q(e) is exactly rae_rank_queries': acc + (add[q] + Ab[e]) with acc the one
 * k-ascending fp32 fmaf chain on v_mfma_f32_32x32x2_f32 (no split-K; this entry runs a
 * copy of the rank kernel's K loop, to be kept identical to it), so both give the same bits for the same (Q row, A row, embed, add, Ab).
 * Candidates of query q: the entities e in [0, n_entities) other than skip[q] (skip NULL or outside
 * [0, n): nothing is skipped) whose score is not NaN.  -0.0f counts and is returned as +0.0f, so
 * the order on scores is the order of float comparison.  Row q of the outputs is its candidates
 * ordered by score descending, then entity ascending (a total order: the output is unique), cut
 * to `top` entries and padded with (-1, -inf); top > n_entities is valid.
 * A query's row is bitwise independent of nq, of its position and of the other queries.  Every
 * pointer is a device pointer except the struct.  Plan-free, stream-ordered, capturable:
 * allocates nothing, never synchronises, writes only ents_out, scores_out and workspace;
 * arguments are checked before the first HIP call.
 * Limits: rae_rank_queries' (nq >= 0, 0 is valid and reads no pointer; 1 <= n_entities < 2^31,
 * 1 <= embed <= 1024, ldq >= embed, ldq % 4 == 0, Q 16-byte aligned, A 16-byte aligned when
 * embed % 4 == 0, workspace 256-byte aligned) and 1 <= top <= 32.  Long query lists run in
 * rounds of 1024.                                                                               */
typedef struct rae_topk_args {
    const float *Q; int64_t ldq; int64_t nq;
    const float *add;           /* (nq) or NULL                                                */
    const int32_t *skip;        /* (nq) or NULL: entity left out of query q                    */
    const float *A, *Ab;        /* (n_entities, embed), (n_entities) or NULL                   */
    int64_t n_entities; int32_t embed;
    int32_t top;                /* 1..32                                                       */
    int32_t *ents_out;          /* (nq, top)                                                   */
    float   *scores_out;        /* (nq, top), may be NULL                                      */
    void *workspace; int64_t workspace_bytes;
} rae_topk_args;
int rae_topk_queries(const rae_topk_args* a, rae_stream_t stream);

/* rae_eval_topk: the `top` best entities for both arguments of rows [row0, row0+nrows) of a split
 * at the current parameters.  Queries and constants are rae_eval_rank's (the table above, query
 * 2b + t - 1 of row b); ents / scores are (nrows, 2, top) with rae_topk_queries' order and padding.
 * skip_true != 0 leaves the row's true entity args_t out of side t, as rae_eval_rank does;
 * skip_true == 0 ranks every entity.  Note for 'sp': side 2's score of args2 is then
 * g_2(args2) = <A[args2], C2 P> + c_2 + Ab[args2], not the objective's positive score u_2 (the
 * reference's A[args1]-twice behaviour, see rae_eval_rank).
 * Reads the fields of `a` that rae_eval_rank reads, with the same shape limits; rows run in rounds
 * of 2048.  Plan-free, stream-ordered, capturable; writes only the outputs and the workspace; a
 * row's outputs are bitwise independent of row0, nrows and the other rows.  nrows == 0 is valid
 * and writes nothing.                                                                           */
typedef struct rae_topk_out {
    int32_t *ents;              /* (nrows, 2, top); not read when nrows == 0                   */
    float   *scores;            /* (nrows, 2, top), may be NULL                                */
    int32_t top;                /* 1..32                                                       */
    int32_t skip_true;          /* != 0: the row's true entity args_t is left out              */
} rae_topk_out;
int rae_eval_topk(const rae_eval_args* a, const rae_topk_out* out, rae_stream_t stream);

/* bytes of workspace of rae_topk_queries (q, with e NULL) or of rae_eval_topk (e, with q NULL) at
 * `top`; host only, no HIP call; -1 on a bad argument or unless exactly one is given.  Reads the
 * shapes only; independent of nq / nrows; depends on n_entities only through the strip count
 * (<= 128).  The strips' lists of one round of 1024 queries, 8 bytes a key: at most 32 MiB at
 * top = 32; rae_eval_topk adds rae_eval_rank's query buffers of one round of rows.             */
int64_t rae_topk_workspace_bytes(const rae_topk_args* q, const rae_eval_args* e, int32_t top);

/* --- relation scores from the decoder: which relation do the two arguments themselves support
 * (no reference counterpart: the reference contracts the encoder's P into the decoder first) ---- */
/* psi_k(e1, e2), a1 = A[e1], a2 = A[e2]:
 *     sp          <C1[:,k], a1> + <C2[:,k], a1>     (the reference's A[args1]-twice behaviour, as the
 *                                                    objective scores it: psi does not depend on e2)
 *     rescal      a1^T R3[:,:,k] a2
 *     rescal+sp   a1^T R3[:,:,k] a2 + <C1[:,k], a1> + <C2[:,k], a2>
 * so sum_k P_k psi_k is rae_eval_rank's `one`; the entity biases are not part of psi.
 * rae_relation_scores: psi_out[q * ldp + k] for nq caller-given pairs; columns [relations, ldp) are
 * never written.  A pair with an id outside [0, n_entities) gets a row of NaN: nothing is read out
 * of range and no other row is disturbed.  Exact fp32 on v_mfma_f32_16x16x4_f32 whatever operands
 * training ran with; the outer product a1 a2^T is formed in registers and never stored.
 * A row's psi is a function of the row's own operands and of (decoder, embed, relations) alone:
 * bitwise independent of nq, of the row's position and of the other rows, and the same from
 * rae_relation_scores and rae_eval_relations for the same (e1, e2).  The contraction is not split:
 * one value is one accumulator chain over the contraction rows (R3's (i, j) rows, then C1's, then
 * C2's) in slabs of TK rows in ascending order, TK = 128 / 64 / 32 for relations <= 16 / <= 128 /
 * above; step s = 4 q + e < TK / 4 of a slab adds its rows 16 q + 4 g + e, g = 0..3, in one
 * instruction: an order fixed by relations alone.  No atomics.
 * Every pointer is a device pointer except the struct.  Plan-free, stream-ordered, capturable:
 * allocates nothing, never synchronises, writes only psi_out (and, rae_eval_relations, its outputs
 * and the workspace); arguments are checked before the first HIP call.  nq == 0 is valid, reads no
 * pointer and writes nothing.
 * Limits: rae_eval_cost's shapes (relations <= 512, a multiple of 4 above 128, <= 320 for the
 * bilinear decoders; embed <= 1024; C1 / C2 / R3 16-byte aligned when relations % 4 == 0); the
 * kernel's own budget adds nothing (at most 84 KiB of LDS, at relations = 320); 1 <= n_entities <
 * 2^31, ldp >= relations.  rae_relation_scores needs no workspace (rae_relscore_workspace_bytes
 * gives 0): workspace may be NULL, and must be 256-byte aligned when it is not.  Long lists run in
 * rounds of 16384 pairs.                                                                        */
typedef struct rae_relscore_args {
    int32_t decoder;            /* RAE_DEC_*                                                   */
    int32_t relations, embed;   /* m, r                                                        */
    int64_t n_entities;
    const float *A, *C1, *C2, *R3;   /* unused ones may be NULL                               */
    const int32_t *e1, *e2;     /* (nq)                                                        */
    int64_t nq;
    float *psi_out; int64_t ldp;
    void *workspace; int64_t workspace_bytes;
} rae_relscore_args;
int rae_relation_scores(const rae_relscore_args* a, rae_stream_t stream);

/* rae_eval_relations: rows [row0, row0+nrows) of a split at the current parameters, (e1, e2) =
 * (args1, args2) of the row.  Per row, with S = x W + Wb:
 *     psi_k                        as above
 *     l_k = logsig(psi_k + Ab[e1]) + logsig(psi_k + Ab[e2])   (rae_eval_cost's pos term at the
 *                                                    one-hot relation k, the same -softplus form)
 *     joint_k = logsoftmax_k(S) + l_k,  the log-softmax as z_k - log sum exp z with z = S - max S
 *               (never the log of a rounded P: finite for every finite logit)
 *     labels_dec = argmax_k psi_k      labels_joint = argmax_k joint_k
 * both the first maximum, NaN counting as the maximum (rae_label's rule).  Any of the four outputs
 * may be NULL, not all of them.  Reads the fields of `a` that rae_eval_rank reads (Ab included);
 * shape limits and alignment as rae_eval_cost.  Rows run in rounds of 16384; when psi is NULL the
 * round's psi lives in the workspace.  A row's outputs are bitwise independent of row0, nrows and
 * the other rows.  nrows == 0 is valid and writes nothing.                                      */
typedef struct rae_rel_out {
    float *psi, *joint;                 /* (nrows, relations), each may be NULL                */
    int64_t *labels_dec, *labels_joint; /* (nrows), each may be NULL                           */
} rae_rel_out;
int rae_eval_relations(const rae_eval_args* a, const rae_rel_out* out, rae_stream_t stream);

/* bytes of workspace of rae_relation_scores (q, with e NULL: 0) or of rae_eval_relations (e, with q
 * NULL: one round's psi and log-softmax); host only, no HIP call; -1 on a bad argument or unless
 * exactly one is given.  Reads the shapes only; independent of nq / nrows.                      */
int64_t rae_relscore_workspace_bytes(const rae_relscore_args* q, const rae_eval_args* e);

/* --- cluster evaluation (get_clusters_sets learning/OieInduction.py:321-340;
 *     evaluation/OieEvaluation.py:23-44,90-127) ------------------------------------ */
/* Plan-free and stream-ordered like rae_label / rae_eval_cost: every pointer is a device
 * pointer, the calls allocate nothing, never synchronise (capturable; the table is zeroed by a
 * kernel) and check their arguments before the first HIP call.  Integer atomics only: the table
 * is bit-exact whatever the form, grid size or arrival order.                               */
#define RAE_CCOUNT_AUTO   0   /* private LDS table per workgroup when it fits, else global      */
#define RAE_CCOUNT_LDS    1   /* workgroup-private LDS counters, flushed once per workgroup     */
#define RAE_CCOUNT_GLOBAL 2   /* integer atomics straight into table                             */
#define RAE_CCOUNT_ACCUMULATE 0x100  /* or-ed into form: add to table (else it is zeroed first) */
/* LDS budget of the LDS form: relations * (n_gold + 1) 32-bit counters <= 16384 (64 KiB of
 * gfx950's 160 KiB per workgroup, so two workgroups stay resident per CU and one streams while
 * the other zeroes or flushes its counters; the flagship 100 x 41 table takes 16 KiB).  AUTO
 * takes the LDS form within the budget; asking for it beyond the budget is RAE_E_INVALID.   */
#define RAE_CCOUNT_LDS_CELLS 16384

/* table[(c)*(n_gold+1) + g] += |{ i < nrows : labels[i] == c, gold[i] == g }|,  column n_gold
 * counts the rows with gold[i] outside [0, n_gold) (unlabelled: -1).  Rows whose label is
 * outside [0, relations) are skipped (never an out-of-range access).  int64 table.
 * relations in [1, 512] (no multiple-of-4 rule), n_gold in [0, 4095], nrows >= 0 (nrows == 0
 * still zeroes the table unless accumulating).  labels / gold need their element alignment
 * only: they are read 16 bytes at a time between a scalar head and tail.                    */
int rae_cluster_count(const int64_t* labels, const int32_t* gold, int64_t nrows,
                      int32_t relations, int32_t n_gold, int32_t form, int64_t* table,
                      rae_stream_t stream);

/* table -> metrics_out[4] = { f1, precision, recall, numberOfElements } (double) with the
 * semantics of rae/evaluation.py compute_metrics;  gold_sizes[g] = |G_g| and n_assessable =
 * |A| are over the WHOLE gold standard of the split (rows that were not labelled -- the
 * dropped tail -- still count there, as in the reference).  sizes_out (relations int64,
 * may be NULL) = cluster sizes incl. unlabelled members (get_clusters_size).
 *   precision = sum n_cg^2 / a_c / |A|, a_c = sum_{g < n_gold} n_cg (a_c == 0 adds nothing)
 *   recall    = sum n_cg^2 / |G_g| / |A|  (|G_g| == 0 adds nothing)
 *   n_assessable == 0 -> (0, 0, 0); f1 = 0 when precision = recall = 0; numberOfElements =
 *   the sum of the whole table; terms are double(n)*double(n)/double(a).
 * One launch, fixed summation order (bitwise reproducible, a function of the table alone):
 * within a cluster row lane j of a wave adds columns j, j + 64, ... in order and the 64 lane
 * sums fold by the xor tree 32, 16, ..., 1; the row sums are then added in cluster order.
 * gold_sizes may be NULL when n_gold == 0.                                                  */
int rae_b3_metrics(const int64_t* table, const int64_t* gold_sizes, int64_t n_assessable,
                   int32_t relations, int32_t n_gold, double* metrics_out,
                   int64_t* sizes_out, rae_stream_t stream);

/* --- per-cluster trigger profiles (Visualizator.print_clusters evaluation/Visuals.py:8-45;
 *     get_example_feature learning/OieData.py:100-106) ------------------------------------ */
/* Plan-free and stream-ordered like the cluster evaluation above: every pointer is a device
 * pointer, no allocation, no synchronisation (capturable), arguments checked before the first
 * HIP call, integer arithmetic only (bit-exact whatever the grid or arrival order).        */

/* keys_out[i] = key_of_feature[f], f the first stored column of row row0 + i (CSR order) with
 * key_of_feature[f] >= 0; -1 when the row has none.  values != NULL: a column whose stored
 * value is 0 is not counted (scipy's nonzero() drops it in the reference).  A column index
 * outside [0, n_features) carries no key (never an out-of-range read).  n_features and nrows in
 * [0, 2^31); nrows == 0 is valid.  Computed once per split: the key is static.             */
int rae_row_keys(const int32_t* indptr, const int32_t* indices, const float* values,
                 const int32_t* key_of_feature, int64_t n_features,
                 int64_t row0, int64_t nrows, int32_t* keys_out, rae_stream_t stream);

/* counts[c * n_keys + k] += |{ i < nrows : labels[i] == c, keys[i] == k }|; rows with a label
 * outside [0, relations) or a key outside [0, n_keys) are skipped (there is no "unlabelled"
 * column: the reference drops None).  The table is zeroed by a kernel first unless
 * accumulate != 0.  relations in [1, 512], n_keys in [1, 2^22], relations * n_keys <= 2^27
 * (512 MiB of counters), 0 <= nrows < 2^31: a cell cannot overflow within one call, and a
 * caller who accumulates keeps the total number of rows below 2^31.  labels / keys need their
 * element alignment only (16-byte reads between a scalar head and tail).  32-bit integer
 * atomics into global memory; the duplicates of a wave instruction are merged first.       */
int rae_cluster_key_count(const int64_t* labels, const int32_t* keys, int64_t nrows,
                          int32_t relations, int32_t n_keys, int32_t accumulate,
                          int32_t* counts, rae_stream_t stream);

/* Row c of the table starts at counts + c * ld (ld >= n_keys); keys_out / counts_out are
 * (relations, top) int32.  A row's output is its cells with count > 0 ordered by count
 * descending, then key ascending (a total order: the output is unique), cut to `top` entries
 * and padded with (-1, 0).  top in [1, 32] (top > n_keys is valid), n_keys in [1, 2^22]; counts
 * up to 2^31 - 1 order correctly.  One pass over each row.                                  */
int rae_cluster_topk(const int32_t* counts, int32_t relations, int32_t n_keys, int64_t ld,
                     int32_t top, int32_t* keys_out, int32_t* counts_out, rae_stream_t stream);

/* --- relation feature profiles: what the encoder's W keys on (no reference counterpart:
 *     get_clusters_with_info dumps raw feature lists and is dead code) ---------------------- */
/* Plan-free and stream-ordered like the entries above: every pointer is a device pointer except
 * the struct itself, no allocation, no synchronisation (capturable), arguments checked before the
 * first HIP call; they write only their outputs and the workspace.                          */

/* support[f] (+)= the number of stored entries (i, f) of rows [row0, row0+nrows) whose value is
 * non-zero (values NULL: every stored entry) -- np.bincount of the kept column indices.  Columns
 * outside [0, n_features) are skipped and never read out of range.  Zeroed by a kernel first
 * unless accumulate != 0.  Integer atomics only: exact whatever the grid or arrival order.
 * 0 <= n_features < 2^31, 0 <= nrows < 2^31 (nrows == 0 still zeroes).  Pointers need their
 * element alignment only.                                                                    */
int rae_feature_support(const int32_t* indptr, const int32_t* indices, const float* values,
                        int64_t n_features, int64_t row0, int64_t nrows, int32_t accumulate,
                        int32_t* support, rae_stream_t stream);

/* Per relation k the `top` best features by score(f, k), of the eligible features f in
 * [0, n_features): support == NULL, or support[f] >= min_support.
 *   centre == 0: score(f, k) = W[f * ldw + k];
 *   centre == 1: score(f, k) = (float)((double)W[f, k] - s_f / (double)relations), one rounding to
 *     fp32, s_f the row sum in double in rae_b3_metrics' order: lane j of 64 adds columns j,
 *     j + 64, ... ascending, the 64 lane sums fold by the xor tree 32, 16, ..., 1.
 * The candidates of relation k are the eligible f whose score is not NaN (-0.0f counts and is
 * returned as +0.0f); row k of feats_out / scores_out ((relations, top)) is its candidates by
 * score descending, then feature ascending (rae_topk_queries' total order: the output is unique),
 * cut to `top` and padded with (-1, -inf).  1 <= relations <= 512 (no multiple-of-4 rule),
 * 0 <= n_features < 2^31 (0: all padding; W may then be NULL), ldw >= relations, 1 <= top <= 32
 * (top > n_features is valid); element offsets into W are 64-bit; W and support need their
 * element alignment only.  A relation's row is bitwise independent of top's padding, of the
 * launch decomposition and of the other relations.                                          */
typedef struct rae_ftopk_args {
    const float* W; int64_t n_features; int32_t relations; int64_t ldw;   /* ldw >= relations   */
    const int32_t* support; int32_t min_support;  /* support NULL: every feature is eligible     */
    int32_t centre;                               /* 0: W[f,k]   1: W[f,k] - mean_f              */
    int32_t top;                                  /* 1..32                                       */
    int32_t* feats_out; float* scores_out;        /* (relations, top); scores_out may be NULL    */
    void* workspace; int64_t workspace_bytes;     /* 256-byte aligned                            */
} rae_ftopk_args;
/* The bytes rae_feature_topk needs for a's n_features, relations, top and centre: the strips'
 * lists (at most 128 strips x relations x top keys of 8 bytes) plus, centred, 8 bytes per
 * feature.  Host only; -1 on a bad argument.                                                */
int64_t rae_feature_topk_workspace_bytes(const rae_ftopk_args* a);
int rae_feature_topk(const rae_ftopk_args* a, rae_stream_t stream);

/* --- cluster exemplars: a cluster's clearest and its boundary rows (no reference counterpart) --- */
/* Plan-free and stream-ordered like the entries above: every pointer is a device pointer except
 * the struct itself, no allocation, no synchronisation (capturable), arguments checked before the
 * first HIP call; they write only their outputs and the workspace.                          */

/* rae_label with the encoder's confidence.  Argument rules and shape limits are rae_label's
 * (relations in [1, 512], a multiple of 4 above 128; W / Wb 16-byte aligned when relations % 4
 * == 0), with row0 >= 0 and 0 <= nrows < 2^31 checked; nrows == 0 writes nothing.  margin_out and
 * pmax_out may each be NULL.  Per row i of [row0, row0+nrows), stored at index i - row0, with
 * S = x W + Wb as rae_label computes it (bitwise):
 *   labels_out  rae_label's label: the first maximum of S, NaN counting as the maximum.
 *   margin_out  S[label] - S[second], one fp32 subtraction; second is the best column among
 *               k != label by the same rule.  relations == 1: +inf.  NaN whenever the subtraction
 *               is (a NaN logit, inf - inf); otherwise >= 0, and 0 on a tie.
 *   pmax_out    bitwise the value rae_label stores at probs[i, label].
 * A row's three outputs are a function of the row and W, Wb, relations alone: bitwise independent
 * of row0, nrows and the other rows.                                                         */
int rae_label_stats(const int32_t* indptr, const int32_t* indices, const float* values,
                    const float* W, const float* Wb, int32_t relations,
                    int64_t row0, int64_t nrows, int64_t* labels_out, float* margin_out,
                    float* pmax_out, rae_stream_t stream);

/* Per cluster c the `top` rows by a per-row score.  The candidates of cluster c are the rows i in
 * [0, nrows) with labels[i] == c whose score is not NaN; rows with a label outside [0, relations)
 * are skipped (never an out-of-range access); -0.0f counts and is returned as +0.0f, +-inf are
 * ordinary scores.  Row c of rows_out / scores_out ((relations, top)) is its candidates by score --
 * descending for largest == 1, ascending for largest == 0 -- then row index ascending (a total
 * order: the output is unique), cut to `top` and padded with (-1, -inf) for either order.  The
 * returned scores are bitwise the input scores (-0 -> +0 aside); rows_out indexes the call's rows,
 * 0 ... nrows - 1.  0 <= nrows < 2^31 (0: all padding; labels / scores may then be NULL),
 * 1 <= relations <= 512, 1 <= top <= 32 (top above a cluster's size is valid).  labels and scores
 * need their element alignment only.  The result is bitwise independent of the launch
 * decomposition, which is a function of (nrows, relations, top) alone.                      */
typedef struct rae_exemplar_args {
    const int64_t* labels; const float* scores; int64_t nrows;   /* 0 <= nrows < 2^31           */
    int32_t relations;                            /* 1..512                                      */
    int32_t top;                                  /* 1..32                                       */
    int32_t largest;                              /* 1: highest scores first   0: lowest first   */
    int32_t* rows_out; float* scores_out;         /* (relations, top); scores_out may be NULL    */
    void* workspace; int64_t workspace_bytes;     /* 256-byte aligned                            */
} rae_exemplar_args;
/* The bytes rae_cluster_exemplars needs for a's nrows, relations and top: the strips' lists, at
 * most 128 strips x 512 x 32 keys of 8 bytes = 16 MiB.  Host only; -1 on a bad argument.    */
int64_t rae_cluster_exemplars_workspace_bytes(const rae_exemplar_args* a);
int rae_cluster_exemplars(const rae_exemplar_args* a, rae_stream_t stream);

/* --- measurement helper (bench.py; no reference counterpart) ------------------------- */
/* STREAM-style device copy of `bytes` (multiple of 16, 16-byte aligned pointers) with float4
 * loads and stores: the measured HBM ceiling bench.py reports next to the 8 TB/s spec.   */
int rae_stream_copy(const void* src_dev, void* dst_dev, int64_t bytes, rae_stream_t stream);
/* bf16 MFMA throughput probe: `blocks` workgroups of 4 waves, each wave `iters` rounds of 8
 * independent v_mfma_f32_16x16x32_bf16 (16384 flops each); writes one float per wave to
 * sink_dev (blocks * 4 floats).  bench.py times it: the measured dense bf16 MFMA ceiling.  */
int rae_mfma_probe(int64_t iters, int32_t blocks, float* sink_dev, rae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RAE_H */
