// What a plan decides, without touching the GPU: plan_resolve validates a rae_config, resolves
// every kernel form and lays out the workspace.  No HIP runtime call and no kernel is named
// here, so the whole of it runs (and is tested, tests/plan_dump.hip) on a machine without a
// GPU; rae_plan_create (rae.hip) allocates, binds the workspace pointers and sets the kernel
// attributes from the resolved spec.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rae.h"
#include "rae_bilinear.hpp"
#include "rae_sp_split.hpp"
#include "rae_common.hpp"
#include "rae_dp.hpp"
#include "rae_index.hpp"
#include "rae_p2p.hpp"
#include "rae_sp.hpp"
#include "rae_step.hpp"
#include "rae_update.hpp"

namespace rae {

__host__ __device__ inline int n_ctiles(int dec, int r, int m) {
    return dec != RAE_DEC_RESCAL ? 2 * ((r + 15) / 16) * ((m + 15) / 16) : 0;
}
// the R-tensor update: one wave per 16 rows (i, j) of R x all m relations (slot nCt + tile)
__host__ __device__ inline int n_rtiles(int dec, int r, int m) {
    return dec != RAE_DEC_SP ? (r * r + 15) / 16 : 0;    // 16 rows of R/C x all m each
}

// Update launch layout (workgroups of RAE_NWAVE = 4 waves), in dispatch order:
//   [0, nT)              one dense 16x16 tile per workgroup: C1/C2 tiles, then Wb tiles
//                        (no row index needed: they start at once; K = batch split 4 ways)
//   [nT, nT + nP)        one wave task each, no row index needed: the cost
//   then, after the batch's index header: one workgroup per very heavy A row, per very heavy
//   W row, and the remaining workgroups' waves grid-stride over the heavy A rows, heavy W
//   rows, light A rows, light W rows (one row per wave)
__host__ __device__ inline int update_wave_free_tasks(int dec, int r, int m) {
    return 1;                                            // the cost (R rows: k_bil_rows)
}
#ifndef RAE_SPLIT_RM
#define RAE_SPLIT_RM 32768    // r*m above which the SP forward runs split (rae_sp_split.hpp)
#endif
#ifndef RAE_ROWPCT
#define RAE_ROWPCT 100        // row-task waves per 100 dispatch-table capacity entries
#endif
#ifndef RAE_HCH
#define RAE_HCH 128           // very heavy rows above this many records are split into chunks
#endif
#ifndef RAE_PRIV_MAXL
#define RAE_PRIV_MAXL 4096    // private rows (auto) below this global batch (equal at 4096)
#endif
#ifndef RAE_HCH_MINL
#define RAE_HCH_MINL 2048     // ... in plans with a global batch of at least this many examples
#endif
#ifndef RAE_NVC_MIN
#define RAE_NVC_MIN 32
#endif
#ifndef RAE_NVC_DIV
#define RAE_NVC_DIV 2         // very heavy row workgroup slots: max(32, L / RAE_NVC_DIV)
#endif
#ifndef RAE_UPD_WGCAP
#define RAE_UPD_WGCAP 6144    // row-task workgroups (grid-stride beyond; 1536 = one resident round)
#endif
#ifndef RAE_PRIV_ROWW
#define RAE_PRIV_ROWW 4       // private rows: row-task waves per example of the global batch
#endif
// own: the share of the global batch's rows this rank updates (1 / G for the partitioned
// data-parallel update: the row grid and the very heavy slots are sized from it)
__host__ __device__ inline int64_t update_grid(int dec, int r, int m, int TC, int NVC, int L,
                                               int priv, int privc, int own) {
    const int nT = n_ctiles(dec, r, m) + (m + 15) / 16;
    const int nP = (update_wave_free_tasks(dec, r, m) + RAE_NWAVE - 1) / RAE_NWAVE;
    int64_t rows = ((int64_t)TC * RAE_ROWPCT / 100 / own + RAE_NWAVE - 1) / RAE_NWAVE;
    // with the private rows (StepArgs::priv) taken per example by leading workgroups, the
    // dispatch table keeps ~5 % of the rows: a smaller row grid, grid-striding when a batch has more
    if (priv) {
        const int64_t pr = ((int64_t)L * RAE_PRIV_ROWW / own + RAE_NWAVE - 1) / RAE_NWAVE;
        if (pr < rows) rows = pr;
    }
    if (RAE_UPD_WGCAP > 0 && rows > RAE_UPD_WGCAP) rows = RAE_UPD_WGCAP;
    return (int64_t)nT + nP + NVC + rows + (priv ? (int64_t)priv_workgroups(privc, L) : 0);
}

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// the SP decoder exchanges wire records between ranks (rae_step.hpp): V1 / V2 / G1 are
// recomputed after the all-gather instead of crossing xGMI (1); with dense partials (2) the
// records carry each rank's partial dC1 / dC2 / dWb block instead of every example's dw1 / dw2
inline int wire_records(const rae_config& c) {
    if (c.decoder != RAE_DEC_SP || c.world_size <= 1) return 0;
    if (c.dp_dense == RAE_DPDENSE_RECORDS) return 1;
    if (c.dp_dense == RAE_DPDENSE_PARTIALS) return 2;
    // partials when their chunk is at most half of dw1 / dw2 (l >~ 2 m): below that they move
    // about as many bytes and k_dpart (~4 us at C3, l = 100) sits on the critical path
    const int pc = align4((dense_partial_floats(c.embed, c.relations) + c.batch_size - 1) /
                          c.batch_size);
    return pc <= align4(c.embed) ? 2 : 1;
}
// the exchange record of a config (rae_exchange_record_floats and the plan share it)
inline RecLayout plan_layout(const rae_config& c) {
    return make_layout(c.decoder, c.relations, c.embed, c.neg_samples, wire_records(c),
                       c.batch_size);
}

// The workspace as an arena: take() reserves a 256-byte-aligned range and records which pointer
// of the spec receives base + offset (by the pointer's byte offset inside the PlanSpec: the spec
// is copied into the plan); bind() patches every recorded pointer once the base is known.  A
// region that is not taken leaves its pointer as it was (null, or the exchange buffer for vb /
// dwb).
struct WsArena {
    struct Bind { size_t field, off; };
    size_t bytes = 0;
    std::vector<Bind> binds;
};

struct PlanSpec {
    StepArgs args;          // every scalar + the caller's pointers; workspace pointers null
    int64_t* d_cursor = nullptr;
    int64_t* d_zero = nullptr;
    int* d_err = nullptr;
    size_t smem_fwd = 0;
    size_t smem_idx = 0;    // k_idx_sort<true> (partitions of more than RAE_IDX_FAST keys)
    size_t smem_idxf = 0;   // k_idx_sort<false>
    size_t smem_dec = 0;
    size_t smem_mt = 0;     // k_bil_mt: one 8 x 16 x m block of R in LDS
    size_t smem_mt0 = 0;    // ... its first pass (no transposed image for dP): less LDS per WG
    bool mt_direct = false; // fp32 blocks beyond LDS (m > 320): k_bil_mt reads R from L2
    bool sp_split = false;  // SP forward as enc -> GEMM -> dec -> GEMM -> fin (large shapes)
    size_t smem_spe = 0;    // k_sp_enc
    size_t smem_spd = 0;    // k_sp_dec (one negative side)
    bool mt_bf16 = false;
    int grid_fwd = 0, grid_update = 0, grid_dense = 0;
    bool v4 = false;
    int q = 1;
    int dp2 = 0;            // bf16 dP kernel: 0 none (bil_gemm_dp*), 1 k_bil_dp2<7,7>, 2 <8,8>
    WsArena arena;

    template <class T>
    void take(T*& field, size_t bytes) {
        arena.binds.push_back({(size_t)((const char*)&field - (const char*)this), arena.bytes});
        arena.bytes += (bytes + 255) & ~size_t(255);
    }
    void bind(char* base) {
        for (const WsArena::Bind& b : arena.binds) {
            char* ptr = base + b.off;
            memcpy((char*)this + b.field, &ptr, sizeof(ptr));
        }
        args.err = d_err;
        args.cursor = d_cursor;
    }
    // the workspace offset a pointer of this spec is bound to, -1 when its region is not taken
    template <class T>
    int64_t ws_offset(T* const& field) const {
        const size_t f = (size_t)((const char*)&field - (const char*)this);
        for (const WsArena::Bind& b : arena.binds)
            if (b.field == f) return (int64_t)b.off;
        return -1;
    }
};

// rae_buffers is read for null-ness only (and copied into args)
inline int plan_resolve(const rae_config& c, const rae_buffers& buf, PlanSpec& s, std::string& err) {
    auto fail = [&err](int code, const std::string& msg) { err = msg; return code; };
    if (c.decoder < 0 || c.decoder > 2) return fail(RAE_E_INVALID, "decoder must be 0..2");
    if (c.optimizer < 0 || c.optimizer > 1) return fail(RAE_E_INVALID, "optimizer must be 0..1");
    if (c.relations < 1 || c.relations > 1024)
        return fail(RAE_E_INVALID, "relations must be in [1, 1024]");
    if (c.embed < 1 || c.embed > 1024) return fail(RAE_E_INVALID, "embed must be in [1, 1024]");
    if (c.neg_samples < 1) return fail(RAE_E_INVALID, "neg_samples must be >= 1");
    if (c.sp_forward < RAE_SPFWD_AUTO || c.sp_forward > RAE_SPFWD_SPLIT ||
        c.bil_dp < RAE_BILDP_AUTO || c.bil_dp > RAE_BILDP_MTILE ||
        c.bil_prep < RAE_BILPREP_AUTO || c.bil_prep > RAE_BILPREP_KERNEL ||
        c.dp_update < RAE_DPUPD_REPLICATED || c.dp_update > RAE_DPUPD_PARTITIONED ||
        c.priv_rows < RAE_PRIV_AUTO || c.priv_rows > RAE_PRIV_ON ||
        c.dp_dense < RAE_DPDENSE_AUTO || c.dp_dense > RAE_DPDENSE_PARTIALS ||
        c.heavy_chunk < RAE_HCHUNK_AUTO || c.heavy_chunk > RAE_HCHUNK_ON ||
        c.dp_xchg < RAE_XCHG_COLLECTIVE || c.dp_xchg > RAE_XCHG_P2P_PIPE)
        return fail(RAE_E_INVALID, "unknown kernel form (sp_forward / bil_dp / bil_prep / dp_update / "
                                   "priv_rows / dp_dense / heavy_chunk / dp_xchg)");
    if (c.dp_xchg != RAE_XCHG_COLLECTIVE &&
        (c.dp_update != RAE_DPUPD_PARTITIONED || c.world_size > 31 || c.embed % 4 ||
         c.relations % 4 || c.embed > 512 || c.relations > 512))
        return fail(RAE_E_INVALID, "the peer-to-peer exchange runs the partitioned update "
                                   "(world_size <= 31; embed and relations multiples of 4, <= 512)");
    // the pipelined form marks a row's reading peers in one byte, and its update pushes rows
    // from the row tasks only (not from the private-row tasks)
    if (c.dp_xchg == RAE_XCHG_P2P_PIPE && (c.world_size > 8 || c.priv_rows == RAE_PRIV_ON))
        return fail(RAE_E_INVALID, "the pipelined peer-to-peer exchange needs world_size <= 8 and "
                                   "private rows off");
    if (c.bil_dp == RAE_BILDP_MTILE && !(c.decoder != RAE_DEC_SP && c.mfma_bf16 && c.relations <= 128))
        return fail(RAE_E_INVALID, "bil_dp MTILE needs a bf16 bilinear plan with relations <= 128");
    if (c.dp_update == RAE_DPUPD_PARTITIONED && (c.lambda1 != 0.f || c.lambda2 != 0.f))
        return fail(RAE_E_INVALID, "the partitioned data-parallel update needs lambda1 = lambda2 = 0 "
                                   "(a regulariser makes every W row change every step)");
    if (c.batch_size < 1 || c.world_size < 1 || c.rank < 0 || c.rank >= c.world_size)
        return fail(RAE_E_INVALID, "bad batch_size/world_size/rank");
    if (c.n_examples < (int64_t)c.batch_size * c.world_size)
        return fail(RAE_E_INVALID, "fewer examples than one global batch");
    if (c.n_entities < 1 || c.n_features < 1 || c.n_entities >= (1ll << 31))
        return fail(RAE_E_INVALID, "bad n_entities / n_features");
    if (!buf.W || !buf.Wb || !buf.A || !buf.Ab || !buf.indptr || !buf.indices ||
        !buf.args1 || !buf.args2 || !buf.exchange || !buf.costs)
        return fail(RAE_E_INVALID, "missing required buffer");
    if (c.decoder != RAE_DEC_RESCAL && (!buf.C1 || !buf.C2))
        return fail(RAE_E_INVALID, "C1/C2 required for this decoder");
    if (c.decoder != RAE_DEC_SP && !buf.R3) return fail(RAE_E_INVALID, "R/C tensor required");
    if (c.optimizer == RAE_OPT_ADAGRAD &&
        (!buf.acc_W || !buf.acc_Wb || !buf.acc_A || !buf.acc_Ab ||
         (c.decoder != RAE_DEC_RESCAL && (!buf.acc_C1 || !buf.acc_C2)) ||
         (c.decoder != RAE_DEC_SP && !buf.acc_R3)))
        return fail(RAE_E_INVALID, "AdaGrad accumulators required");

    s = PlanSpec();
    StepArgs& a = s.args;
    memset(&a, 0, sizeof(a));
    a.lay = plan_layout(c);
    // 2^30 floats, not 2^31: RecBuf::load (rae_common.hpp) addresses a record through a raw
    // buffer resource whose offsets are 32-bit BYTE offsets from the buffer's base, so a record
    // at or beyond 4 GiB would wrap
    if ((int64_t)a.lay.rec * c.batch_size * c.world_size >= (1ll << 30) ||
        (int64_t)3 * align4(c.embed) * c.batch_size * c.world_size >= (1ll << 30))
        return fail(RAE_E_INVALID, "exchange buffer exceeds 2^30 floats = 4 GiB, the range of its "
                                   "32-bit byte offsets (global batch too large)");
    const int L = c.batch_size * c.world_size;
    const int NJ = 2 + 2 * c.neg_samples;
    a.dec = c.decoder;
    a.opt = c.optimizer;
    a.N = c.n_examples;
    a.d = c.n_features;
    a.n = c.n_entities;
    a.m = c.relations;
    a.r = c.embed;
    a.s = c.neg_samples;
    a.l = c.batch_size;
    a.L = L;
    a.rank = c.rank;
    a.lr = c.learning_rate;
    a.alpha = c.alpha;
    // adjust = batch / N_train (learning/OieInduction.py:131) with the GLOBAL batch
    const double adjust = (double)L / (double)c.n_examples;
    a.l1adj = (float)(c.lambda1 * adjust);
    a.l2adj = (float)(c.lambda2 * adjust);
    a.invD = (float)(1.0 / (4.0 * L + 2.0 * L * c.neg_samples));
    a.ext_reg = c.ext_reg;
    a.reg_on = (c.lambda1 != 0.f || c.lambda2 != 0.f) ? 1 : 0;
    a.indptr = buf.indptr;
    a.indices = buf.indices;
    a.values = buf.values;
    a.args1 = buf.args1;
    a.args2 = buf.args2;
    a.neg1 = buf.neg1;
    a.neg2 = buf.neg2;
    a.neg_mode = c.neg_mode;
    a.neg_stride = c.neg_stride;
    a.W = buf.W; a.Wb = buf.Wb; a.A = buf.A; a.Ab = buf.Ab;
    a.C1 = buf.C1; a.C2 = buf.C2; a.R3 = buf.R3;
    a.aW = buf.acc_W; a.aWb = buf.acc_Wb; a.aA = buf.acc_A; a.aAb = buf.acc_Ab;
    a.aC1 = buf.acc_C1; a.aC2 = buf.acc_C2; a.aR3 = buf.acc_R3;
    a.ex = buf.exchange;
    // the update's record vectors: in the records, or (wire record) the vector buffer
    a.vb = a.ex;
    a.vbs = a.lay.rec;
    a.vG1 = a.lay.oG1; a.vV1 = a.lay.oV1; a.vV2 = a.lay.oV2; a.vG2 = a.lay.oG2;
    if (a.lay.wire) {
        const int r4 = align4(c.embed);
        a.vbs = 3 * r4;
        a.vV1 = 0; a.vV2 = r4; a.vG1 = 2 * r4; a.vG2 = 0;
    }
    // the forward's dw1 / dw2: in the records, or (dense partials) a rank-local buffer
    a.dpart = a.lay.wire == 2 ? 1 : 0;
    a.dwb = a.ex;
    a.dws = a.lay.rec;
    a.dw1o = a.lay.odw1; a.dw2o = a.lay.odw2;
    if (a.dpart) {
        a.dws = 2 * align4(c.embed);
        a.dw1o = 0; a.dw2o = align4(c.embed);
    }
    a.costs = buf.costs;
    s.v4 = (c.relations % 4 == 0) && (c.embed % 4 == 0);
    {
        const int vw = s.v4 ? 4 : 1;
        const int qa = ceil_div(c.embed / vw, 64), qm = ceil_div(c.relations / vw, 64);
        const int q = qa > qm ? qa : qm;
        if (q > 2)
            return fail(RAE_E_INVALID,
                        "relations/embed are limited to 512 (128 when not multiples of 4)");
        s.q = q <= 1 ? 1 : 2;
    }

    // row-index partitions: ~1024 records per partition on average, LDS holds RAE_KCAP
    a.RA = L * NJ;
    a.RW = c.max_batch_nnz > 0 ? c.max_batch_nnz : 1;
    a.HA = index_partitions(a.RA);
    a.HW = index_partitions(a.RW);
    a.G = c.world_size;
    a.part = c.dp_update == RAE_DPUPD_PARTITIONED ? 1 : 0;
    if (a.HA > RAE_IDX_HMAX || a.HW > RAE_IDX_HMAX)
        return fail(RAE_E_INVALID, "global batch too large for the row index (more than " +
                                   std::to_string(RAE_IDX_HMAX * RAE_IDX_PART) +
                                   " records of one table)");
    {
        const int64_t nb = c.n_examples / L;
        // partitioned: the peers' row lists take 2 G (LA + LW) ints per slot -> a shorter window
        int64_t win = c.index_window > 0 ? c.index_window : (a.part ? 256 : 2048);
        if (win > nb) win = nb;
        a.index_window = win < 1 ? 1 : win;
    }
    int bbits = 1;
    while ((1 << bbits) < L) ++bbits;
    a.posbits = 31 - bbits;
    if (c.max_row_nnz >= (1 << a.posbits))
        return fail(RAE_E_INVALID, "an example has too many features for the record encoding");
    // parameter / dense-row partial slots for the regulariser
    a.nregC = n_ctiles(c.decoder, c.embed, c.relations) + n_rtiles(c.decoder, c.embed, c.relations);
    s.grid_dense = 1024;
    a.nregW = a.reg_on ? s.grid_dense : 0;

    // workspace
    s.take(s.d_cursor, 8); s.take(s.d_zero, 8); s.take(s.d_err, 8); s.take(a.base_cost, 8);
    const size_t W_ = (size_t)a.index_window;
    s.take(a.srecA, 4ull * W_ * a.RA); s.take(a.urowA, 16ull * W_ * a.RA);
    s.take(a.srecW, 4ull * W_ * a.RW); s.take(a.urowW, 16ull * W_ * a.RW);
    s.take(a.skeyA, 8ull * W_ * a.RA); s.take(a.skeyW, 8ull * W_ * a.RW);
    s.take(a.gidx, 4ull * W_ * 4 * RAE_IDX_HMAX);
    s.take(a.pcls, 16ull * W_ * 2 * RAE_IDX_HMAX);
    a.VCA = a.RA / (RAE_VHEAVY + 1) + 1;       // very heavy rows per batch are fewer than this
    a.VCW = a.RW / (RAE_VHEAVY + 1) + 1;
    // the update's dispatch table: every unique row is at most one task (TC = records), and
    // NVC very heavy rows get a workgroup each (L / RAE_NVC_DIV, at least 32 -- the rest run as
    // wave tasks)
    a.TC = a.RA + a.RW;
    {
        const int Lo = a.part ? (L + a.G - 1) / a.G : L;     // the rows this rank updates
        const int nvc = Lo / RAE_NVC_DIV > RAE_NVC_MIN ? Lo / RAE_NVC_DIV : RAE_NVC_MIN;
        a.NVC = nvc < a.VCA + a.VCW ? nvc : a.VCA + a.VCW;
        // large global batches: very heavy rows with at least 2 RAE_HCH records split into
        // floor(records / RAE_HCH) chunks (every chunk a workgroup task: NVC >= HF + 1 >
        // records / RAE_HCH, the most chunks a batch can have -- rae_index.hpp build_batch_tasks)
        a.hch = (c.heavy_chunk == RAE_HCHUNK_ON ||
                 (c.heavy_chunk == RAE_HCHUNK_AUTO && L >= RAE_HCH_MINL)) ? RAE_HCH : 0;
        if (a.hch) {
            a.HF = (a.RA + a.RW) / a.hch + 1;
            if (a.NVC < a.HF + 1) a.NVC = a.HF + 1;
            a.hps = ((c.embed + 3) & ~3) + 4 > ((c.relations + 3) & ~3) ? ((c.embed + 3) & ~3) + 4
                                                                       : ((c.relations + 3) & ~3);
        }
    }
    s.take(a.thdr, 16 * W_); s.take(a.task, 16ull * W_ * a.TC);
    s.take(a.vtask, 16ull * W_ * a.NVC);
    if (a.hch) {
        s.take(a.hfin, 16ull * W_ * a.HF);
        s.take(a.hpart, 4ull * a.NVC * a.hps);
    }
    {
        int cap = c.max_row_nnz > 0 ? c.max_row_nnz : 1;
        if (cap > 256) cap = 256;                    // the fast path's feature capacity
        a.dcap = cap;
        a.dstride = ((2 + NJ + cap) + 31) & ~31;      // whole 128-B lines per example
    }
    // private rows (rows one record of the global batch references, updated per example by the
    // update launch): plans without a regulariser whose record slots fit one wave (NJ <= 64);
    // the example's features from its descriptor (<= dcap, <= 32).  Several ranks: every rank's
    // update takes the private rows it updates (replicated: all; partitioned: its own), so the
    // descriptors cover the whole global batch
    // auto: single-rank and replicated plans below a global batch of RAE_PRIV_MAXL; at larger
    // batches and in the partitioned update (a rank's own private rows: a few per example) the
    // row tasks do them faster (profiles/r04_ab.txt)
    const bool priv_ok = !a.reg_on && NJ <= 64;
    a.priv = (priv_ok && (c.priv_rows == RAE_PRIV_ON ||
                          (c.priv_rows == RAE_PRIV_AUTO && !a.part && L < RAE_PRIV_MAXL))) ? 1 : 0;
    a.dnx = (a.priv && c.world_size > 1) ? L : c.batch_size;
    a.d0 = a.dnx == L ? c.rank * c.batch_size : 0;
    s.take(a.desc, 4ull * W_ * a.dnx * a.dstride);
    s.take(a.regpart, 16ull * (a.nregC + a.nregW + 1));
    if (a.reg_on) s.take(a.gWs, 4ull * c.n_features * c.relations);
    // partitioned data-parallel update: list capacities are the worst cases of one rank's
    // l examples (every entity id distinct; the largest global batch's features)
    a.LA = a.part ? c.batch_size * NJ : 0;
    a.LW = a.part ? a.RW : 0;
    if (a.part) {
        s.take(a.dpl, 4ull * W_ * dpl_slot_ints(a.G, a.LA, a.LW));
        s.take(a.dpc, 4ull * W_ * 2 * a.G * 2);
    }
    s.take(a.dpmax, 16);
    // peer-to-peer exchange: the peers' mapped buffers and this rank's expected signal counts
    a.xchg = c.dp_xchg;
    a.p2p_timeout = RAE_P2P_TIMEOUT_DEFAULT;
    s.take(a.peers, sizeof(PeerBufs) * (size_t)c.world_size);
    s.take(a.p2p_expect, 4ull * 2 * c.world_size);
    // pipelined peer-to-peer form: two parities of row-mark bytes over the owned rows
    a.pipe = (c.dp_xchg == RAE_XCHG_P2P_PIPE && c.world_size > 1) ? 1 : 0;
    a.pmA = a.pipe ? (int)((((c.n_entities + c.world_size - 1) / c.world_size + 3) / 4 + 3) & ~3) : 0;
    a.pmW = a.pipe ? (int)((((c.n_features + c.world_size - 1) / c.world_size + 3) / 4 + 3) & ~3) : 0;
    if (a.pipe) s.take(a.pm, 4ull * 2 * (a.pmA + a.pmW));
    const bool bil = c.decoder != RAE_DEC_SP;
    a.bf16 = (bil && c.mfma_bf16) ? 1 : 0;
    // dP contraction form: in the second M-tile pass (bf16, m <= 128) by default; k_bil_dp2
    // (bf16, LDS-staged R slices: the C5 shape compiled exactly, others up to r = 256, m = 128
    // padded; float4 rows) or the strided k_bil_dp otherwise / on request
    const bool mt_ok = bil && c.mfma_bf16 && c.relations <= 128;
    const bool c5 = (c.embed + 31) / 32 == 7 && (c.relations + 15) / 16 == 7;
    const bool dp2_ok = a.bf16 && c.embed % 4 == 0 && c.relations % 4 == 0 &&
                        (c5 || (c.embed <= 256 && c.relations <= 128));
    const bool mtdp = mt_ok && (c.bil_dp == RAE_BILDP_AUTO || c.bil_dp == RAE_BILDP_MTILE);
    if (!mtdp && dp2_ok && c.bil_dp != RAE_BILDP_STRIDED) s.dp2 = c5 ? 1 : 2;
    a.nib = bil ? (s.dp2 ? (c.embed + RAE_IB2 - 1) / RAE_IB2 : (c.embed + RAE_IB - 1) / RAE_IB) : 0;
    a.r4 = align4(c.embed);
    const int64_t nbi_mt = (c.embed + RAE_MTI - 1) / RAE_MTI, nbj_mt = (c.embed + RAE_MTJ - 1) / RAE_MTJ;
    a.nmtp = (int)(nbi_mt * nbj_mt);
    if (bil) {
        s.take(a.dPpart, 4ull * a.nib * c.batch_size * c.relations);
        s.take(a.mtV, 4ull * nbj_mt * c.batch_size * a.r4);
        s.take(a.mtW, 4ull * nbi_mt * c.batch_size * a.r4);
    }
    if (mtdp) s.take(a.mtP, 4ull * a.nmtp * c.batch_size * c.relations);
    // split SP forward (rae_sp_split.hpp) for runtime shapes whose decoder matrices stream
    // through every example's workgroup (r*m > RAE_SPLIT_RM; C4: 90 k), or on request
    s.sp_split = !bil && (c.sp_forward == RAE_SPFWD_SPLIT ||
                          (c.sp_forward == RAE_SPFWD_AUTO &&
                           (int64_t)c.embed * c.relations > RAE_SPLIT_RM));
    a.spss = sps_stride(c.embed);
    if (s.sp_split) s.take(a.sps, 4ull * a.spss * c.batch_size);
    a.privnf = a.priv ? (a.dcap < 32 ? a.dcap : 32) : 0;
    a.privc = (a.priv && a.part && c.world_size > 1) ? 1 : 0;
    if (a.priv) s.take(a.pmask, 16ull * W_ * L);
    a.Lp = (L + 31) / 32 * 32;
    a.fuse_prep = (a.bf16 && c.world_size == 1 && c.bil_prep == RAE_BILPREP_AUTO) ? 1 : 0;
    if (a.bf16) s.take(a.facT, 16ull * c.embed * a.Lp);
    if (a.lay.wire) s.take(a.vb, 4ull * a.vbs * L);
    if (a.dpart) s.take(a.dwb, 4ull * a.dws * L);
    if (a.bf16) s.take(a.pfrag, 16ull * (a.Lp / 32) * ((c.relations + 15) / 16) * 64);

    // k_idx_sort<big>: keys, scan scratch, segment starts (the fast form: RAE_IDX_FAST keys)
    s.smem_idx = 8ull * RAE_KCAP + 4ull * 64 + 4ull * RAE_KCAP;
    s.smem_idxf = 8ull * RAE_IDX_FAST + 4ull * 64 + 4ull * RAE_IDX_FAST;
    s.smem_fwd = 4ull * example_smem_floats(c.decoder, c.relations, c.embed, c.neg_samples);
    s.smem_spe = s.sp_split ? 4ull * example_smem_floats(0, c.relations, c.embed, 0) : 0;
    s.smem_spd = s.sp_split ? 4ull * sp_dec_side_smem_floats(c.embed, c.neg_samples) : 0;
    s.smem_dec = bil ? 4ull * bil_dec_smem_floats(c.embed, c.neg_samples) : 0;
    // the M-tile passes: bf16 blocks need m <= 128 (four K steps of 32 per fragment set)
    s.mt_bf16 = bil && a.bf16 && c.relations <= 128;
    s.smem_mt = bil ? bil_mt_lds_bytes(c.relations, s.mt_bf16) : 0;
    // the first pass never stages the transposed image (dP rides on the second): with half the
    // LDS, two of its workgroups fit a CU and all (r/8)(r/16) start at once
    s.smem_mt0 = (bil && s.mt_bf16) ? (size_t)RAE_MTI * RAE_MTJ * (((c.relations + 31) / 32 * 32) + 8) * 2
                                    : s.smem_mt;
    if (s.smem_mt > RAE_MT_LDS_MAX) {        // fp32 block too large to stage (m > 320)
        s.mt_direct = true;
        s.smem_mt = 0;
    }
    if (s.smem_fwd > 160 * 1024 || s.smem_idx > 160 * 1024 || s.smem_dec > 160 * 1024)
        return fail(RAE_E_INVALID, "configuration needs more than 160 KiB LDS per example "
                                   "workgroup (relations / embed / neg_samples too large)");
    s.grid_fwd = c.batch_size;
    const int64_t gu = update_grid(c.decoder, c.embed, c.relations, a.TC, a.NVC, L, a.priv,
                                   a.privc, a.part ? a.G : 1);
    if (gu >= (1ll << 31)) return fail(RAE_E_INVALID, "update grid too large");
    s.grid_update = (int)gu;
    return RAE_OK;
}

}  // namespace rae
