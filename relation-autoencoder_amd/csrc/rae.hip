// MI355X (gfx950) relation-autoencoder training path: kernels + C ABI (include/rae.h).
//
// Per training step (one func['train'] call of learning/OieInduction.py:189):
//   SP:        k_forward  one workgroup per example: encoder + decoder forward/backward
//                         (rae_sp.hpp) -> exchange record
//   bilinear:  k_bil_enc -> k_bil_mt (MFMA) -> k_bil_dec -> k_bil_mt (MFMA) -> k_bil_dp (MFMA)
//              -> k_bil_fin
//                         (rae_bilinear.hpp) -> exchange record
//   (the per-batch row index is built ahead, a window of batches at a time: k_idx_count ->
//    k_idx_scatter -> k_idx_sort -> k_build_tasks, rae_index.hpp)
//   [caller all-gathers the exchange records across data-parallel ranks]
//   k_update   one wavefront per distinct referenced row / dense decoder row / bias:
//              deterministic gradient sums + AdaGrad/SGD in place (rae_update.hpp)
//   k_dense_w + k_finalize_cost   only when lambda1/lambda2 != 0 (dense W regulariser)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "../../include/rae.h"
#include "rae_bilinear.hpp"
#include "rae_cluster.hpp"
#include "rae_sp_split.hpp"
#include "rae_common.hpp"
#include "rae_dp.hpp"
#include "rae_eval.hpp"
#include "rae_index.hpp"
#include "rae_label.hpp"
#include "rae_p2p.hpp"
#include "rae_profile.hpp"
#include "rae_rank.hpp"
#include "rae_relscore.hpp"
#include "rae_topk.hpp"
#include "rae_feature.hpp"
#include "rae_exemplar.hpp"
#include "rae_sampler.hpp"
#include "rae_sp.hpp"
#include "rae_step.hpp"
#include "rae_update.hpp"
#include "rae_plan.hpp"

using namespace rae;

#define RAE_VERSION 1
#ifndef RAE_UPD_WPE
#define RAE_UPD_WPE 5   // SP update: <= 102 VGPRs -> 20 waves per CU (6: 85 VGPRs spilled the
                        // Q = 2 rows of C4 -- 23.8 vs 20.2 us update; r03_ab.txt)
#endif

// ======================================================================================
// kernels
// ======================================================================================
template <bool V4, class D>
__global__ __launch_bounds__(RAE_FBT) __attribute__((amdgpu_waves_per_eu(1, 2)))
void k_forward(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t g = step_batch(a);
    if constexpr (FastSP<D>::ok) sp_example_fast<D>(a, g, blockIdx.x, smem);
    else sp_example<V4, D>(a, g, blockIdx.x, smem);
}

// ---- split SP forward for large runtime shapes (rae_sp_split.hpp) ----
template <bool V4>
__global__ __launch_bounds__(RAE_FBT) void k_sp_enc(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    sp_split_enc<V4>(a, step_batch(a), blockIdx.x, smem);
}
template <bool VEC>
__global__ __launch_bounds__(RAE_BT) void k_sp_cp(StepArgs a) {
    __shared__ __attribute__((aligned(16))) float red[RAE_BT * 4];
    sp_split_cp<VEC>(a, blockIdx.x, red);
}
template <bool V4>
__global__ __launch_bounds__(RAE_FBT) void k_sp_dec(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    sp_split_dec<V4>(a, step_batch(a), blockIdx.x / RAE_SPD_NP, blockIdx.x % RAE_SPD_NP, smem);
}
template <bool VEC>
__global__ __launch_bounds__(RAE_DW_BT) void k_sp_ctdw(StepArgs a) {
    __shared__ __attribute__((aligned(16))) float red[RAE_DW_BT * 4 + 16];
    sp_split_ctdw<VEC>(a, blockIdx.x, red);
}
// SP dense partials (data parallel): this rank's dC1 / dC2 / dWb into its records, before the exchange
__global__ __launch_bounds__(RAE_BT) void k_dpart(StepArgs a) {
    __shared__ __attribute__((aligned(16))) rae_f4 sacc[RAE_BT];
    dpart_tile(a, blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63, sacc);
}
// SP wire record (data parallel): V1, V2, G1 of the whole global batch after the exchange
template <bool VEC>
__global__ __launch_bounds__(RAE_BT) void k_vrec(StepArgs a) {
    const int t = blockIdx.x * RAE_NWAVE + (threadIdx.x >> 6);
    if (t < vrec_tasks(a.L, a.r)) sp_vrec<VEC>(a, t, threadIdx.x & 63);
}

// ---- RESCAL / RESCAL+SP forward phase (rae_bilinear.hpp) ----
template <bool V4>
__global__ __launch_bounds__(RAE_FBT) void k_bil_enc(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bil_encode<V4>(a, step_batch(a), blockIdx.x, smem);
}
template <class D>
__global__ __launch_bounds__(RAE_FBT) void k_bil_enc_fast(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bil_encode_fast<D>(a, step_batch(a), blockIdx.x, smem);
}
#ifdef RAE_MT_WPE      // A/B: occupancy target of the M-tile passes (waves per SIMD)
#define RAE_MT_ATTR __attribute__((amdgpu_waves_per_eu(RAE_MT_WPE)))
#else
#define RAE_MT_ATTR
#endif
template <bool BF16, bool DIRECT = false, bool DP = true>
__global__ __launch_bounds__(RAE_MTT) RAE_MT_ATTR void k_bil_mt(StepArgs a, int pass) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bil_mt<BF16, DIRECT, DP>(a, pass, smem);
}
template <bool V4>
__global__ __launch_bounds__(RAE_DBT) void k_bil_dec(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bil_decode<V4>(a, step_batch(a), blockIdx.x, smem);
}
__host__ __device__ inline int bil_dp_tasks(int l, int m, int nib) {
    return ((l + 15) / 16) * ((m + 15) / 16) * nib;
}
template <bool BF16>
__global__ __launch_bounds__(RAE_BT) void k_bil_dp(StepArgs a) {
    const int t = blockIdx.x * RAE_NWAVE + (threadIdx.x >> 6);
    if (t >= bil_dp_tasks(a.l, a.m, a.nib)) return;
    if constexpr (BF16) bil_gemm_dp_bf16(a, t, threadIdx.x & 63);
    else bil_gemm_dp(a, t, threadIdx.x & 63);
}
template <int NJS, int MT>
__global__ __launch_bounds__((dp2_threads<NJS, MT>())) void k_bil_dp2(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bil_gemm_dp2<NJS, MT>(a, blockIdx.x, smem);
}
__global__ __launch_bounds__(RAE_BT) void k_bil_prep(StepArgs a) { bil_prep(a); }
// the R-tensor update: one wave per 16 rows (i, j) of R x all m relations (slot nCt + tile)
template <int OPT, bool LDS>
__global__ __launch_bounds__(RAE_BT) void k_bil_rows(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * RAE_NWAVE + w;
    if (t >= n_rtiles(a.dec, a.r, a.m)) return;
    const int slot = n_ctiles(a.dec, a.r, a.m) + t;
    if constexpr (LDS)
        task_bilinear_rows_lds<OPT>(a, t, slot, threadIdx.x & 63,
                                    reinterpret_cast<float*>(smem) + (size_t)w * (OPT == 0 ? 2 : 1) * 16 * a.m);
    else
        task_bilinear_rows<OPT>(a, t, slot, threadIdx.x & 63);
}
__global__ __launch_bounds__(RAE_FINT) void k_bil_fin(StepArgs a) {
    __shared__ float sdp[1024];          // NS * m <= max(RAE_FINT, m) <= 1024
    __shared__ float smt[4 * 1024];      // M-tile half sums, r <= 1024
    __shared__ float red[2 * RAE_FINW];
    bil_finish(a, blockIdx.x, sdp, smt, red);
}

// shapes with compile-time specialisations of the forward kernel (BASELINE.json configs
// C3/C5: K=100 r=200 s=20; C2: K=30 r=100 s=10); every other shape runs the runtime-shape
// instantiation of the same code
typedef FixDims<100, 200, 20> DimsC3;
typedef FixDims<30, 100, 10> DimsC2;

// row index of global batches [first, first + gridDim.x) (rae_index.hpp): blockIdx.y = table
// (0 A / Ab, 1 W; 2: the example descriptors), blockIdx.z = slice of RAE_IDX_EPS examples or
// hash partition
__global__ __launch_bounds__(RAE_BT) void k_idx_count(StepArgs a, int64_t first) {
    __shared__ int sh[RAE_IDX_HMAX + RAE_IDX_EPS + 1];
    const int64_t g = first + blockIdx.x;
    if (blockIdx.y == 2) {
        build_batch_desc<RAE_BT>(a, g, g % a.index_window, blockIdx.z);
        return;
    }
    index_count<RAE_BT>(a, g, g % a.index_window, blockIdx.y, blockIdx.z, sh);
}
__global__ __launch_bounds__(RAE_BT) void k_idx_scatter(StepArgs a, int64_t first) {
    __shared__ int sh[2 * RAE_IDX_HMAX + RAE_IDX_EPS + 1 + 32];
    const int64_t g = first + blockIdx.x;
    index_scatter<RAE_BT>(a, g, g % a.index_window, blockIdx.y, blockIdx.z, sh);
}
template <bool BIG>
__global__ __launch_bounds__(RAE_FBT) void k_idx_sort(StepArgs a, int64_t first) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t g = first + blockIdx.x;
    index_sort<RAE_FBT, BIG>(a, g, g % a.index_window, blockIdx.y, blockIdx.z, smem);
}
// the update's dispatch tables of the same batches (after k_idx_sort): blockIdx.y = range of
// RAE_TASK_PER table entries
__global__ __launch_bounds__(RAE_BT) void k_build_tasks(StepArgs a, int64_t first) {
    __shared__ int sh[6 * (RAE_IDX_HMAX + 1)];
    const int64_t g = first + blockIdx.x;
    build_batch_tasks<RAE_BT>(a, g, g % a.index_window, blockIdx.y, sh);
}

// partitioned data-parallel update (rae_dp.hpp): the peers' row lists of global batches
// [first, first + gridDim.x); blockIdx.y = peer, blockIdx.z = direction * 2 + table
__global__ __launch_bounds__(RAE_FBT) void k_build_dplists(StepArgs a, int64_t first) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t g = first + blockIdx.x;
    build_dp_list<RAE_FBT>(a, g, g % a.index_window, blockIdx.z >> 1, blockIdx.y, blockIdx.z & 1,
                           smem);
}
// peer-to-peer exchange (rae_p2p.hpp)
__global__ __launch_bounds__(RAE_BT) void k_p2p_recs(StepArgs a) { p2p_push_records(a); }
__global__ __launch_bounds__(RAE_BT) void k_p2p_rows(StepArgs a) { p2p_push_rows(a); }
__global__ __launch_bounds__(RAE_BT) void k_p2p_pre(StepArgs a, int prologue, int nmb) {
    p2p_pre(a, prologue, nmb);
}
__global__ __launch_bounds__(64) void k_p2p_signal(StepArgs a, int kind) { p2p_signal(a, kind); }
__global__ __launch_bounds__(64) void k_p2p_wait(StepArgs a, int kind, unsigned per) {
    p2p_wait(a, kind, per);
}
template <bool PACK>
__global__ __launch_bounds__(RAE_BT) void k_dp_move(StepArgs a) {
    const int64_t t = (int64_t)blockIdx.x * RAE_NWAVE + (threadIdx.x >> 6);
    dp_move<PACK>(a, t, threadIdx.x & 63);
}

#ifdef RAE_STAMPS
#define RAE_WAVE_END()                                                                      \
    do {                                                                                    \
        if (a.stamps && lane == 0)      /* end of the wave's LAST task */                    \
            a.stamps[(size_t)gw * 4 + 2] = __builtin_amdgcn_s_memrealtime();                 \
    } while (0)
#else
#define RAE_WAVE_END() do { } while (0)
#endif

#ifndef RAE_ROWS_FIRST
#define RAE_ROWS_FIRST 0      // update: dispatch the row tasks ahead of the dense tiles
#endif
#ifndef RAE_PRIV_LAST
#define RAE_PRIV_LAST 1       // private-row workgroups dispatched after every other update task
#endif

// LDS of one update workgroup: workgroup tasks' partials (a row: Q vectors per lane, or a tile:
// 4 floats per lane, per wave) + the Ab partials
template <bool V4, int Q>
__host__ __device__ constexpr int update_lds_floats() {
    return (RAE_NWAVE * Q * RAE_WAVE * (V4 ? 4 : 1) > RAE_NWAVE * RAE_WAVE * 4
                ? RAE_NWAVE * Q * RAE_WAVE * (V4 ? 4 : 1) : RAE_NWAVE * RAE_WAVE * 4) + RAE_NWAVE;
}

// wg0 / ngrid: this workgroup's index and the number of workgroups of the update's own grid
// (the fused bilinear kernel puts the update's workgroups in front of the R-tile ones)
// VS: where the A-row tasks find the record vectors (rae_update.hpp entity_accum): 0 SP records
// (single rank), 1 bilinear records, 2 the SP wire record's vector buffer (data parallel)
template <int OPT, bool V4, int Q, int VS, bool PP = false>
__device__ __forceinline__ void update_body(const StepArgs& a, int wg0, int ngrid, float* lds) {
    typedef typename VecT<V4>::T VT;
    constexpr int kF = update_lds_floats<V4, Q>() - RAE_NWAVE;
    float* sgb = lds + kF;
    VT* spart = reinterpret_cast<VT*>(lds);
    const int lane = threadIdx.x & 63;
    // wave / workgroup indices as provably uniform values: every task index, row id and
    // record offset derived from them is then scalar (s_load of the segment, SGPR soffsets,
    // scalar branches) instead of VGPR-resident and exec-masked
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int wgp = __builtin_amdgcn_readfirstlane(wg0);
    const int gw = wgp * RAE_NWAVE + w;
    const int64_t g = step_batch(a);
    if (a.priv) {                 // private rows: (RAE_PRA + 1) L workgroups (1 per example when
                                  // compact), dispatched first (RAE_PRIV_LAST 0) or last
        const int nX = priv_workgroups(a.privc, a.L);
        const int x = RAE_PRIV_LAST ? wgp - (ngrid - nX) : wgp;
        if (x >= 0 && x < nX) {
            task_private_rows<OPT, V4, Q, VS>(a, g, x, w, lane);
            return;
        }
        if (!RAE_PRIV_LAST) wgp -= nX;
        ngrid -= nX;
    }
    const int64_t ex0 = g * (int64_t)a.L;
    const int mt = (a.m + 15) / 16, rt = (a.r + 15) / 16;
    const int nCt = n_ctiles(a.dec, a.r, a.m);
    const int nT = nCt + mt;
    const int nPt = update_wave_free_tasks(a.dec, a.r, a.m);
    const int nP = (nPt + RAE_NWAVE - 1) / RAE_NWAVE;
    // logical task order: tiles, cost, very heavy rows, row waves; RAE_ROWS_FIRST dispatches the
    // row part first (physical order: very heavy rows, row waves, tiles, cost)
    int wg = wgp;
    if (RAE_ROWS_FIRST) {
        const int nrow = ngrid - nT - nP;
        wg = wgp < nrow ? nT + nP + wgp : wgp - nrow;
    }
    const int64_t slot = g % a.index_window;
#ifdef RAE_STAMPS
    unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
#define RAE_FIRST(kind_)                                                                    \
    do {                                                                                    \
        if (a.stamps && lane == 0) {                                                        \
            a.stamps[(size_t)gw * 4 + 0] = t_start;                                         \
            a.stamps[(size_t)gw * 4 + 1] = (unsigned long long)(kind_);                     \
        }                                                                                   \
    } while (0)
#else
#define RAE_FIRST(kind_) do { } while (0)
#endif
    if (wg < nT) {                                            // dense tiles
        RAE_FIRST(wg < nCt ? 0 : 2);
        if (VS == 2 && a.dpart) {        // dense partials: the ranks' sums (wave 0), no K chain
            if (w == 0) {
                if (wg < nCt) {
                    const int which = wg / (rt * mt), ti = wg - which * rt * mt;
                    tile_from_partials<OPT>(a, which ? a.C2 : a.C1, which ? a.aC2 : a.aC1, a.r, false,
                                            which * a.r * a.m, (ti / mt) * 16, (ti % mt) * 16, wg, lane);
                } else {
                    tile_from_partials<OPT>(a, a.Wb, a.aWb, 1, true, 2 * a.r * a.m, 0,
                                            (wg - nCt) * 16, 0, lane);
                }
            }
            RAE_WAVE_END();
            return;
        }
        if (wg < nCt) {
            const int which = wg / (rt * mt), ti = wg - which * rt * mt;
            wg_tile<OPT>(a, which ? a.C2 : a.C1, which ? a.aC2 : a.aC1, a.r,
                         which ? a.lay.odw2 : a.lay.odw1, false, (ti / mt) * 16, (ti % mt) * 16,
                         wg, w, lane, reinterpret_cast<rae_f4*>(spart));
        } else {
            wg_tile<OPT>(a, a.Wb, a.aWb, 1, 0, true, 0, (wg - nCt) * 16, 0, w, lane,
                         reinterpret_cast<rae_f4*>(spart));
        }
        RAE_WAVE_END();
        return;
    }
    if (wg < nT + nP) {                                       // the cost (one workgroup)
        if (wg == nT) {
            RAE_FIRST(3);
            task_cost(a, w, lane, reinterpret_cast<double*>(lds));
        }
        RAE_WAVE_END();
        return;
    }
    // row tasks from the slot's dispatch table (build_batch_tasks): the task entry and the
    // table header are loaded together -- one round trip from wave start to the row's segment
    const int u = wg - nT - nP;
    const int4* thp = reinterpret_cast<const int4*>(a.thdr) + slot;
    if (u < a.NVC) {                                          // very heavy rows
        int4 seg = reinterpret_cast<const int4*>(a.vtask)[slot * a.NVC + u];
        const int4 th = *thp;
        if (u >= th.y) return;
        const bool isA = seg.x >= 0;
        RAE_FIRST(isA ? 8 : 9);
        if (isA) {
            wg_entity_row<OPT, V4, Q, VS, PP>(a, slot, seg, w, lane, spart, sgb);
        } else {
            seg.x = ~seg.x;
            wg_feature_row<OPT, V4, Q, PP>(a, ex0, slot, seg, w, lane, spart);
        }
        RAE_WAVE_END();
        return;
    }
    // wave tasks: a wave with several (large global batches: the grid's row part is capped
    // near one resident wave per slot) loads its next task's segment while it works on the
    // current one
    const int nw = (ngrid - nT - nP - a.NVC) * RAE_NWAVE;
    const int4* tk = reinterpret_cast<const int4*>(a.task) + slot * a.TC;
    int t = (u - a.NVC) * RAE_NWAVE + w;
    int4 seg = tk[t < a.TC ? t : a.TC - 1];
    const int T = thp->x;
    for (; t < T; t += nw) {
        int4 cur = seg;
        if (t + nw < T) seg = tk[t + nw];
        const bool curA = cur.x >= 0;
        if (!curA) cur.x = ~cur.x;
        RAE_FIRST((curA ? 4 : 5) + (cur.z - cur.y > RAE_HEAVY ? 2 : 0));
        if (curA) task_entity_row<OPT, V4, Q, VS, PP>(a, slot, cur, lane);
        else task_feature_row<OPT, V4, Q, PP>(a, ex0, slot, cur, lane);
        RAE_WAVE_END();
    }
#undef RAE_FIRST
}

// SP and bilinear variants (the bilinear R-row tasks need more registers).
#if RAE_UPD_WPE > 0
#define RAE_UPD_ATTR __attribute__((amdgpu_waves_per_eu(RAE_UPD_WPE, RAE_UPD_WPE)))
#else
#define RAE_UPD_ATTR
#endif
template <int OPT, bool V4, int Q, bool WIRE>
__global__ __launch_bounds__(RAE_BT) RAE_UPD_ATTR void k_update(StepArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[update_lds_floats<V4, Q>()];
    update_body<OPT, V4, Q, WIRE ? 2 : 0, WIRE>(a, blockIdx.x, gridDim.x, lds);
    if (WIRE && a.pipe) p2p_stores_done();   // the row pushes acknowledged before the wave ends
}
template <int OPT, bool V4, int Q, bool PP = false>
__global__ __launch_bounds__(RAE_BT) void k_update_bil(StepArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[update_lds_floats<V4, Q>()];
    update_body<OPT, V4, Q, 1, PP>(a, blockIdx.x, gridDim.x, lds);
    if (PP && a.pipe) p2p_stores_done();
}
// The bilinear decoders' update phase in ONE launch: workgroups [0, gu) run k_update_bil's tasks
// (Wb tiles, cost, A / W rows: latency-bound chains), the rest k_bil_rows' R tiles (16 rows
// (i, j) x all m per wave: the HBM-heavy R sweep) -- the two have no data in common, so the
// row chains run under the R sweep instead of after it.  Dynamic LDS: the R tiles' (DMA'd R and
// accumulator rows); an update workgroup carves its partials from the same allocation.
template <int OPT, bool V4, int Q, bool PP = false>
__global__ __launch_bounds__(RAE_BT) void k_bil_update(StepArgs a, int gu) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wg = __builtin_amdgcn_readfirstlane(blockIdx.x);
    if (wg < gu) {
        update_body<OPT, V4, Q, 1, PP>(a, wg, gu, reinterpret_cast<float*>(smem));
        if (PP && a.pipe) p2p_stores_done();
        return;
    }
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = (wg - gu) * RAE_NWAVE + w;
    if (t >= n_rtiles(a.dec, a.r, a.m)) return;
    const int slot = n_ctiles(a.dec, a.r, a.m) + t;
    task_bilinear_rows_lds<OPT>(a, t, slot, threadIdx.x & 63,
                                reinterpret_cast<float*>(smem) + (size_t)w * (OPT == 0 ? 2 : 1) * 16 * a.m);
}
#ifndef RAE_BIL_FUSED_UPD
#define RAE_BIL_FUSED_UPD 1   // bilinear update phase as one launch (k_bil_update)
#endif

// rows split into chunks (StepArgs::hch): each row's chunk sums combined in order + its update
template <int OPT, bool V4, int Q, bool PP = false>
__global__ __launch_bounds__(RAE_BT) void k_heavy_fin(StepArgs a) {
    heavy_fin<OPT, V4, Q, PP>(a, blockIdx.x * RAE_NWAVE + (threadIdx.x >> 6), threadIdx.x & 63);
    if (PP && a.pipe) p2p_stores_done();
}

// Dense W sweep (lambda1/lambda2 != 0): g = sparse-part scratch + l1adj*sgn(W) + 2*l2adj*W,
// reset the scratch, L1/L2 partials of the old W per block (fixed grid -> deterministic).
template <int OPT>
__global__ __launch_bounds__(RAE_BT) void k_dense_w(StepArgs a) {
    __shared__ double red[2 * RAE_NWAVE];
    const int64_t total = a.d * (int64_t)a.m;
    double l1 = 0.0, l2 = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)RAE_BT + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * RAE_BT) {
        const float w = a.W[i];
        const float gg = a.gWs[i] + a.l1adj * sgnf(w) + 2.f * a.l2adj * w;
        a.gWs[i] = 0.f;
        l1 += fabsf(w);
        l2 += (double)w * w;
        float ac = (OPT == 0) ? a.aW[i] : 0.f;
        a.W[i] = opt_update<OPT>(w, &ac, gg, a.lr);
        if (OPT == 0) a.aW[i] = ac;
    }
    l1 = wave_sum_d(l1);
    l2 = wave_sum_d(l2);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[2 * w] = l1;
        red[2 * w + 1] = l2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int i = 0; i < RAE_NWAVE; ++i) {
            s1 += red[2 * i];
            s2 += red[2 * i + 1];
        }
        const int slot = a.nregC + blockIdx.x;
        a.regpart[2 * slot] = s1;
        a.regpart[2 * slot + 1] = s2;
    }
}

// cost = base + lambda1*adjust*L1 + lambda2*adjust*L2   (learning/OieInduction.py:134-135)
__global__ void k_finalize_cost(StepArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double L1 = 0.0, L2 = 0.0;
    if (a.ext_reg)
        for (int i = 0; i < a.nregC; ++i) {
            L1 += a.regpart[2 * i];
            L2 += a.regpart[2 * i + 1];
        }
    for (int i = 0; i < a.nregW; ++i) {
        L1 += a.regpart[2 * (a.nregC + i)];
        L2 += a.regpart[2 * (a.nregC + i) + 1];
    }
    const int64_t batch = step_batch(a);
    a.costs[batch] = (float)((double)*a.base_cost + (double)a.l1adj * L1 + (double)a.l2adj * L2);
}

// STREAM-style copy (measurement helper): 4 float4 nontemporal loads in flight per lane
// before the stores, one 1024-vector block per workgroup -- the fastest of the forms
// tools/probes/stream_probe.hip measured on MI355X (5.88 TB/s at 2 GiB)
typedef float rae_v4f __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_stream_copy(const rae_v4f* __restrict__ src,
                                                     rae_v4f* __restrict__ dst, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 1024;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += stride) {
        rae_v4f v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t k = i + 256 * u;
            if (k < n) v[u] = __builtin_nontemporal_load(src + k);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t k = i + 256 * u;
            if (k < n) __builtin_nontemporal_store(v[u], dst + k);
        }
    }
}

// bf16 MFMA throughput probe (measurement helper): every wave runs `iters` rounds of 8
// independent v_mfma_f32_16x16x32_bf16 chains (enough in flight to cover the dependent-issue
// latency), operands in registers, one result per wave stored so nothing is dead code
__global__ __launch_bounds__(256) void k_mfma_probe(int64_t iters, float* sink) {
    typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
    typedef float f4 __attribute__((ext_vector_type(4)));
    bf8 x, y;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        x[e] = (__bf16)(1e-3f * (float)((threadIdx.x + e) & 7));
        y[e] = (__bf16)(1e-3f * (float)((threadIdx.x * 3 + e) & 7));
    }
    f4 acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = f4{0.f, 0.f, 0.f, 0.f};
    for (int64_t it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, acc[c], 0, 0, 0);
    }
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) t += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    if ((threadIdx.x & 63) == 0) sink[blockIdx.x * 4 + (threadIdx.x >> 6)] = t;
}

// ---- forward-only objective (rae_eval.hpp) ----
template <bool V4>
__global__ __launch_bounds__(RAE_EV_BT) void k_eval_dec(EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    eval_dec<V4>(a, reinterpret_cast<float*>(smem));
}
template <bool V4>
__global__ __launch_bounds__(RAE_EV_BT) void k_eval_enc(EvalArgs a) { eval_enc<V4>(a); }
template <bool V4>
__global__ __launch_bounds__(RAE_EV_MTT) void k_eval_mt(EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    eval_mt<V4>(a, reinterpret_cast<float*>(smem));
}
__global__ __launch_bounds__(RAE_EV_BT) void k_eval_blocksum(const float* terms, int n,
                                                             double* partial) {
    __shared__ double red[RAE_EV_NW * 3];
    eval_blocksum(terms, n, partial, red);
}
// sums[c] (+)= the chunk's partials in block order (init: the first chunk sets)
__global__ void k_eval_acc(const double* partial, int nblk, double* sums, int init) {
    const int c = threadIdx.x;
    if (blockIdx.x != 0 || c >= 3) return;
    double t = init ? 0.0 : sums[c];
    for (int b = 0; b < nblk; ++b) t += partial[b * 3 + c];
    sums[c] = t;
}

// ---- argument ranking over all entities (rae_rank.hpp) ----
template <bool V4>
__global__ __launch_bounds__(RAE_EV_BT) void k_rank_build(EvalArgs a, RankBuild o) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    rank_build<V4>(a, o, reinterpret_cast<float*>(smem));
}
__global__ void k_rank_zero(int32_t* greater, int32_t* equal, int nq) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) { greater[q] = 0; equal[q] = 0; }
}
template <bool AV4, bool LSE>
__global__ __launch_bounds__(RAE_RK_BT) void k_rank(RankArgs a) {
    __shared__ float sQ[RAE_RK_TQ * RAE_RK_LDK];
    __shared__ float sA[RAE_RK_TE * RAE_RK_LDK];
    __shared__ float sAb[RAE_RK_TE];
    __shared__ float2 sPart[RAE_RK_TQ];
    rank_scores<AV4, LSE>(a, sQ, sA, sAb, sPart);
}
// lse[q] of the chunk: the strips' (max, sum) pairs merged in strip order
__global__ void k_rank_finish(const float2* part, int strips, int nq, float* lse) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    float m = -INFINITY, s = 0.f;
    for (int t = 0; t < strips; ++t) {
        const float2 o = part[(int64_t)t * RAE_RK_QCHUNK + q];
        rank_lse_merge(m, s, o.x, o.y);
    }
    lse[q] = m == -INFINITY ? -INFINITY : m + logf(s);
}
__global__ __launch_bounds__(RAE_EV_BT) void k_rank_blocksum(const int32_t* greater,
                                                             const int32_t* equal,
                                                             const float* target, const float* lse,
                                                             int n, RankHits hk, double* partial) {
    __shared__ double red[RAE_EV_NW * RAE_RK_NSUM];
    rank_blocksum(greater, equal, target, lse, n, hk, partial, red);
}
// summary[c] (+)= the chunk's partials in block order (init: the first chunk sets)
__global__ void k_rank_acc(const double* partial, int nblk, double* summary, int init) {
    const int c = threadIdx.x;
    if (blockIdx.x != 0 || c >= RAE_RK_NSUM) return;
    double t = init ? 0.0 : summary[c];
    for (int b = 0; b < nblk; ++b) t += partial[b * RAE_RK_NSUM + c];
    summary[c] = t;
}

// ---- top-k entity retrieval (rae_topk.hpp) ----
template <bool AV4>
__global__ __launch_bounds__(RAE_RK_BT) void k_topk(RankArgs a, TopkOut o) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    topk_scores<AV4>(a, o, smem);
}
__global__ __launch_bounds__(RAE_ETK_FQ * 64) void k_topk_finish(const rae_key64* keys, int strips,
                                                                  int nq, int top, int32_t* ents,
                                                                  float* scores) {
    __shared__ rae_key64 sList[RAE_ETK_FQ * 32];
    topk_finish(keys, strips, nq, top, ents, scores, sList);
}

// ---- relation scores from the decoder (rae_relscore.hpp) ----
template <int NTA, int NTB, int TK>
__global__ __launch_bounds__(RAE_RS_BT) void k_relscore(RelArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    rel_scores<NTA, NTB, TK>(a, reinterpret_cast<float*>(smem));
}
__global__ __launch_bounds__(RAE_RS_EBT) void k_rel_enc(RelEnc a) { rel_enc(a); }
__global__ __launch_bounds__(RAE_RS_EBT) void k_rel_fin(RelFin a) { rel_fin(a); }

__global__ void k_add_cursor(int64_t* cursor, int64_t count) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *cursor += count;
}
__global__ void k_set_cursor(int64_t* cursor, int64_t v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *cursor = v;
}

// ======================================================================================
// host side / C ABI
// ======================================================================================
static thread_local std::string g_last_error;

static int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess)                                                              \
            return fail(RAE_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));       \
    } while (0)

// the resolved spec (rae_plan.hpp: args, forms, geometry, workspace layout) + what creation
// and the calls after it add
struct rae_plan : PlanSpec {
    rae_config cfg;
    rae_buffers buf;
    int64_t cursor_moves = 0;  // host count of rae_set_cursor / rae_advance_cursor calls
    int* h_err = nullptr;   // pinned host word of rae_check_on
    unsigned* d_sig = nullptr;  // peer-to-peer signal counters (own allocation: IPC-exported)
    bool peers_set = false;     // rae_set_peer called for every other rank
    int peers_mask = 0;
    char* ws = nullptr;
    unsigned long long* stamps_fwd = nullptr;
#ifdef RAE_WSTAMPS
    unsigned long long* stamps_wave = nullptr;
#endif
    unsigned long long* stamps_upd = nullptr;
    hipEvent_t t_start = nullptr, t_stop = nullptr;   // armed by rae_time_next for ONE call
};

// Main-step launches go through here.  With a timing pair armed (rae_time_next) the kernels
// are launched by hipExtLaunchKernelGGL: the start event takes the first kernel's dispatch
// begin timestamp, the stop event the last kernel's end timestamp -- the kernels' execution
// span as rocprofv3 --kernel-trace reports it, without the event packets' own overhead.
#define RAE_LAUNCH(p, K, g, b, sh, st, ...)                                                 \
    do {                                                                                  \
        if ((p)->t_stop) {                                                                \
            hipEvent_t e0_ = (p)->t_start;                                                \
            (p)->t_start = nullptr;                                                       \
            hipExtLaunchKernelGGL(K, g, b, sh, st, e0_, (p)->t_stop, 0, __VA_ARGS__);      \
        } else {                                                                          \
            hipLaunchKernelGGL(K, g, b, sh, st, __VA_ARGS__);                             \
        }                                                                                 \
    } while (0)

// compile-time dispatch: f gets the runtime value as a std::integral_constant (RAE_CV reads it).
// Kernels are instantiated in the order the launch code first names them (true / 1 / AdaGrad
// first), and the device code follows that order down to the inliner's choices: a change of
// the nesting below is a change of the code object (compare the disassembly).
#define RAE_CV(x) decltype(x)::value
template <class F> static void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}
template <class F> static void with_q(int q, F&& f) {          // row slots per lane: 1 or 2
    if (q == 1) f(std::integral_constant<int, 1>{}); else f(std::integral_constant<int, 2>{});
}
template <class F> static void with_opt(int opt, F&& f) {      // RAE_OPT_ADAGRAD 0 / RAE_OPT_SGD 1
    if (opt == RAE_OPT_ADAGRAD) f(std::integral_constant<int, 0>{});
    else f(std::integral_constant<int, 1>{});
}
template <class F> static void with_vm(int vm, F&& f) {        // k_fsupport's values mode: 0, 1 or 2
    if (vm == 0) f(std::integral_constant<int, 0>{});
    else if (vm == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}

extern "C" const char* rae_last_error(void) { return g_last_error.c_str(); }
extern "C" int rae_version(void) { return RAE_VERSION; }
#ifndef RAE_BUILD_ID
#define RAE_BUILD_ID "unversioned"
#endif
// a diagnostic build (phase stamps, tools/phase_stamps.py) says so in its id: the Python
// binding loads such a library only when RAE_LIB names it explicitly
#ifdef RAE_DIAG
#define RAE_BUILD_KIND "diag-"
#else
#define RAE_BUILD_KIND ""
#endif
__attribute__((used)) static const char g_build_id[] = "RAE_BUILD_ID:" RAE_BUILD_KIND RAE_BUILD_ID;
extern "C" const char* rae_build_id(void) { return g_build_id + 13; }

extern "C" int64_t rae_exchange_record_floats(const rae_config* cfg) {
    if (!cfg) return -1;
    return plan_layout(*cfg).rec;
}
extern "C" int64_t rae_exchange_floats(const rae_config* cfg) {
    if (!cfg) return -1;
    return rae_exchange_record_floats(cfg) * (int64_t)cfg->batch_size * cfg->world_size;
}

// large dynamic LDS is opted into per kernel
static void plan_set_kernel_attributes(const rae_plan* p) {
    auto lds = [](const void* f, size_t bytes) {
        (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    };
    const void* fwd[] = {(const void*)k_forward<true, DimsC3>, (const void*)k_forward<false, DimsC2>,
                         (const void*)k_forward<true, DynDims>, (const void*)k_forward<false, DynDims>,
                         (const void*)k_bil_enc<true>, (const void*)k_bil_enc<false>,
                         (const void*)k_bil_enc_fast<DimsC3>,
                         (const void*)k_sp_dec<true>, (const void*)k_sp_dec<false>};
    for (const void* f : fwd) lds(f, p->smem_fwd);
    if (p->sp_split) {
        lds((const void*)k_sp_enc<true>, p->smem_spe);
        lds((const void*)k_sp_enc<false>, p->smem_spe);
    }
    if (p->cfg.decoder != RAE_DEC_SP) {
        lds((const void*)k_bil_dp2<7, 7>, dp2_lds_bytes<7, 7>());
        lds((const void*)k_bil_dp2<8, 8>, dp2_lds_bytes<8, 8>());
        lds((const void*)k_bil_mt<true>, p->smem_mt);
        lds((const void*)k_bil_mt<true, false, false>, p->smem_mt);
        lds((const void*)k_bil_mt<false>, p->smem_mt);
        lds((const void*)k_bil_dec<true>, p->smem_dec);
        lds((const void*)k_bil_dec<false>, p->smem_dec);
    }
    lds((const void*)k_idx_sort<true>, p->smem_idx);
    lds((const void*)k_build_dplists, 4 * RAE_DPL_KEYS + 4 * 32);
}

// resolve (rae_plan.hpp: every check, form and the workspace layout; nothing is allocated for a
// config that is rejected) -> allocate -> bind -> kernel attributes.  A failure after the plan
// exists leaves through rae_plan_destroy.
extern "C" int rae_plan_create(const rae_config* cfg, const rae_buffers* buf, rae_plan** out) {
    if (!cfg || !buf || !out) return fail(RAE_E_INVALID, "null argument");
    PlanSpec spec;
    std::string err;
    if (const int rc = plan_resolve(*cfg, *buf, spec, err)) return fail(rc, err);
    rae_plan* p = new rae_plan();
    static_cast<PlanSpec&>(*p) = spec;
    p->cfg = *cfg;
    p->buf = *buf;
    auto bail = [p](const char* what, hipError_t e) {
        rae_plan_destroy(p);
        return fail(RAE_E_HIP, e == hipSuccess ? std::string(what)
                                               : std::string(what) + ": " + hipGetErrorString(e));
    };
    const size_t bytes = p->arena.bytes;
    hipError_t e = hipMalloc(&p->ws, bytes);
    if (e != hipSuccess) return bail("hipMalloc workspace", e);
    (void)hipMemset(p->ws, 0, bytes);
    e = hipHostMalloc(reinterpret_cast<void**>(&p->h_err), sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) return bail("hipHostMalloc", e);
    *p->h_err = 0;
    if (cfg->dp_xchg != RAE_XCHG_COLLECTIVE) {
        // the peers add to these words over xGMI and this rank polls them: uncached (no L2
        // line of them can go stale; rae_p2p.hpp "Visibility across GPUs")
        const size_t sb = 4ull * 2 * cfg->world_size;
        e = hipExtMallocWithFlags(reinterpret_cast<void**>(&p->d_sig), sb, hipDeviceMallocUncached);
        if (e == hipSuccess) e = hipMemset(p->d_sig, 0, sb);
        if (e != hipSuccess) return bail("hipMalloc signals", e);
    }
    p->bind(p->ws);
    plan_set_kernel_attributes(p);
    StepArgs& a = p->args;
    a.sig = p->d_sig;
    if (a.sig) {                 // this rank's own entry of the peer table
        const PeerBufs own{a.ex, a.W, a.A, a.Ab, a.sig};
        if (hipMemcpy(a.peers + cfg->rank, &own, sizeof(own), hipMemcpyHostToDevice) != hipSuccess)
            return bail("peer table", hipSuccess);
    }
    *out = p;
    return RAE_OK;
}

extern "C" int rae_plan_forms(const rae_plan* p, rae_config* out) {
    if (!p || !out) return fail(RAE_E_INVALID, "null argument");
    const bool bil = p->cfg.decoder != RAE_DEC_SP;
    out->sp_forward = bil ? 0 : (p->sp_split ? RAE_SPFWD_SPLIT : RAE_SPFWD_FUSED);
    out->bil_dp = !bil ? 0 : (p->args.mtP ? RAE_BILDP_MTILE
                              : (p->dp2 ? RAE_BILDP_STAGED : RAE_BILDP_STRIDED));
    out->bil_prep = (!bil || !p->args.bf16) ? 0 : (p->args.fuse_prep ? RAE_BILPREP_AUTO
                                                                    : RAE_BILPREP_KERNEL);
    out->dp_update = p->cfg.dp_update;
    out->priv_rows = p->args.priv ? RAE_PRIV_ON : RAE_PRIV_OFF;
    out->dp_dense = p->args.lay.wire == 2 ? RAE_DPDENSE_PARTIALS
                  : (p->args.lay.wire == 1 ? RAE_DPDENSE_RECORDS : 0);
    out->heavy_chunk = p->args.hch ? RAE_HCHUNK_ON : RAE_HCHUNK_OFF;
    out->dp_xchg = p->cfg.dp_xchg;
    return RAE_OK;
}

extern "C" int rae_plan_destroy(rae_plan* p) {
    if (!p) return RAE_OK;
    if (p->ws) (void)hipFree(p->ws);
    if (p->h_err) (void)hipHostFree(p->h_err);
    if (p->d_sig) (void)hipFree(p->d_sig);
    delete p;
    return RAE_OK;
}

extern "C" int rae_set_negatives(rae_plan* p, const int32_t* n1, const int32_t* n2, int32_t mode,
                                 int64_t stride) {
    if (!p || !n1 || !n2) return fail(RAE_E_INVALID, "null argument");
    if (mode != RAE_NEG_PER_CALL && mode != RAE_NEG_PER_EPOCH)
        return fail(RAE_E_INVALID, "bad negatives mode");
    p->args.neg1 = n1;
    p->args.neg2 = n2;
    p->args.neg_mode = mode;
    p->args.neg_stride = stride;
    return RAE_OK;
}

extern "C" int rae_set_cursor(rae_plan* p, int64_t batch, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    hipLaunchKernelGGL(k_set_cursor, dim3(1), dim3(64), 0, (hipStream_t)stream, p->d_cursor, batch);
    ++p->cursor_moves;
    HIPCHK(hipGetLastError());
    return RAE_OK;
}
extern "C" int rae_advance_cursor(rae_plan* p, int64_t count, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    hipLaunchKernelGGL(k_add_cursor, dim3(1), dim3(64), 0, (hipStream_t)stream, p->d_cursor, count);
    ++p->cursor_moves;
    HIPCHK(hipGetLastError());
    return RAE_OK;
}
extern "C" int64_t rae_cursor_moves(const rae_plan* p) { return p ? p->cursor_moves : -1; }

static void launch_fwd_sp(rae_plan* p, const StepArgs& a, hipStream_t st) {
    const dim3 gr(p->grid_fwd), bt(RAE_FBT);
    if (p->sp_split) {
        const dim3 gcp(sp_cp_tasks(a.l, a.r)), gct(sp_ctdw_tasks(a.l, a.m));   // WG per tile
        const dim3 gsd(RAE_SPD_NP * p->grid_fwd);          // a workgroup per (example, piece)
        with_bool(p->v4, [&](auto V) { RAE_LAUNCH(p, k_sp_enc<RAE_CV(V)>, gr, bt, p->smem_spe, st, a); });
        with_bool(a.m % 4 == 0, [&](auto V) { RAE_LAUNCH(p, k_sp_cp<RAE_CV(V)>, gcp, dim3(RAE_BT), 0, st, a); });
        with_bool(p->v4, [&](auto V) { RAE_LAUNCH(p, k_sp_dec<RAE_CV(V)>, gsd, bt, p->smem_spd, st, a); });
        with_bool(a.r % 4 == 0,
                  [&](auto V) { RAE_LAUNCH(p, k_sp_ctdw<RAE_CV(V)>, gct, dim3(RAE_DW_BT), 0, st, a); });
        return;
    }
    const bool c3 = a.m == 100 && a.r == 200 && a.s == 20;
    const bool c2 = a.m == 30 && a.r == 100 && a.s == 10;
    if (c3 && p->v4)
        RAE_LAUNCH(p, (k_forward<true, DimsC3>), gr, bt, p->smem_fwd, st, a);
    else if (c2 && !p->v4)
        RAE_LAUNCH(p, (k_forward<false, DimsC2>), gr, bt, p->smem_fwd, st, a);
    else if (p->v4)
        RAE_LAUNCH(p, (k_forward<true, DynDims>), gr, bt, p->smem_fwd, st, a);
    else
        RAE_LAUNCH(p, (k_forward<false, DynDims>), gr, bt, p->smem_fwd, st, a);
}

static void launch_fwd_dp(rae_plan* p, const StepArgs& a, hipStream_t st);
template <bool V4>
static void launch_fwd_bil(rae_plan* p, const StepArgs& a, hipStream_t st) {
    const dim3 ge(p->grid_fwd);
    if (V4 && a.dec == RAE_DEC_RESCAL && a.m == 100 && a.r == 200 && a.s == 20)     // C5 shape
        RAE_LAUNCH(p, (k_bil_enc_fast<DimsC3>), ge, dim3(RAE_FBT), p->smem_fwd, st, a);
    else
        RAE_LAUNCH(p, (k_bil_enc<V4>), ge, dim3(RAE_FBT), p->smem_fwd, st, a);
    const dim3 gmt(((a.r + RAE_MTI - 1) / RAE_MTI) * ((a.r + RAE_MTJ - 1) / RAE_MTJ));
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) RAE_LAUNCH(p, (k_bil_dec<V4>), ge, dim3(RAE_DBT), p->smem_dec, st, a);
        if (p->mt_bf16 && pass == 0)       // no dP: the lighter instantiation, half the LDS
            RAE_LAUNCH(p, (k_bil_mt<true, false, false>), gmt, dim3(RAE_MTT), p->smem_mt0, st, a, pass);
        else if (p->mt_bf16) RAE_LAUNCH(p, (k_bil_mt<true>), gmt, dim3(RAE_MTT), p->smem_mt, st, a, pass);
        else if (p->mt_direct) RAE_LAUNCH(p, (k_bil_mt<false, true>), gmt, dim3(RAE_MTT), 0, st, a, pass);
        else RAE_LAUNCH(p, (k_bil_mt<false>), gmt, dim3(RAE_MTT), p->smem_mt, st, a, pass);
    }
    if (!a.mtP) launch_fwd_dp(p, a, st);              // else dP came with the second pass
    RAE_LAUNCH(p, k_bil_fin, ge, dim3(RAE_FINT), 0, st, a);
}

static void launch_fwd_dp(rae_plan* p, const StepArgs& a, hipStream_t st) {
    const int gd = ceil_div(bil_dp_tasks(a.l, a.m, a.nib), RAE_NWAVE);
    const size_t lds77 = dp2_lds_bytes<7, 7>(), lds88 = dp2_lds_bytes<8, 8>();
    if (p->dp2 == 1)
        RAE_LAUNCH(p, (k_bil_dp2<7, 7>), dim3(a.nib), dim3(dp2_threads<7, 7>()), lds77, st, a);
    else if (p->dp2 == 2)
        RAE_LAUNCH(p, (k_bil_dp2<8, 8>), dim3(a.nib), dim3(dp2_threads<8, 8>()), lds88, st, a);
    else
        with_bool(a.bf16, [&](auto B) { RAE_LAUNCH(p, k_bil_dp<RAE_CV(B)>, dim3(gd), dim3(RAE_BT), 0, st, a); });
}

// peer-to-peer exchange grids (every rank the same: the peers expect these many signals)
static unsigned p2p_rows_grid(const StepArgs& a) {
    const int64_t g = ((int64_t)a.G * (a.capA + a.capW) + RAE_NWAVE - 1) / RAE_NWAVE;
    return (unsigned)(g < 1 ? 1 : g);
}
static unsigned p2p_recs_grid(const StepArgs& a) {
    const int64_t g = ((int64_t)a.l * a.lay.rec / 4 + RAE_BT - 1) / RAE_BT;
    return (unsigned)(g < 1 ? 1 : g);
}
static bool p2p_on(const rae_plan* p) { return p->args.xchg != RAE_XCHG_COLLECTIVE && p->args.G > 1; }
// k_p2p_pre's grid: marking threads (one per list entry of every list, the own one included)
// + pushing waves (one per entry of the peers' lists)
static int p2p_pre_mark_blocks(const StepArgs& a) {
    const int64_t n = (int64_t)a.G * (a.capA + a.capW);
    return (int)((n + RAE_BT - 1) / RAE_BT);
}

static int launch_forward(rae_plan* p, const int64_t* cursor, int64_t off, hipStream_t st) {
    if (!p->args.neg1 || !p->args.neg2) return fail(RAE_E_STATE, "negatives not set");
    StepArgs a = p->args;
    a.cursor = cursor;
    a.step_offset = off;
    a.stamps = p->stamps_fwd;
#ifdef RAE_WSTAMPS
    a.wstamps = p->stamps_wave;
#endif
    const bool p2p = p2p_on(p);
    if (p2p) {
        if (!p->peers_set) return fail(RAE_E_STATE, "peer buffers not set (rae_set_peer)");
        if (!a.pipe) {        // the owned rows the peers' examples read, into their replicas
            const unsigned gr = p2p_rows_grid(a);   // (>= 1 workgroup: the signal follows anyway)
            RAE_LAUNCH(p, k_p2p_rows, dim3(gr), dim3(RAE_BT), 0, st, a);
            RAE_LAUNCH(p, k_p2p_signal, dim3(1), dim3(64), 0, st, a, 1);
        }                     // pipelined: pushed and signalled by the previous step / prologue
        RAE_LAUNCH(p, k_p2p_wait, dim3(1), dim3(64), 0, st, a, 1, 1u);
    }
    if (a.dec == RAE_DEC_SP) {
        launch_fwd_sp(p, a, st);
        if (a.dpart)          // this rank's dense partials into its records, before the exchange
            RAE_LAUNCH(p, k_dpart, dim3(dpart_tasks(a.r, a.m)), dim3(RAE_BT), 0, st, a);
    }
    else with_bool(p->v4, [&](auto V) { launch_fwd_bil<RAE_CV(V)>(p, a, st); });
    if (p2p)                  // this rank's records into every peer's exchange buffer
    {
        // (pipelined: + blocks clearing the next batch's row marks)
        RAE_LAUNCH(p, k_p2p_recs, dim3(p2p_recs_grid(a) + (a.pipe ? 64 : 0)), dim3(RAE_BT), 0, st, a);
        RAE_LAUNCH(p, k_p2p_signal, dim3(1), dim3(64), 0, st, a, 0);
        if (a.pipe) {         // the next batch's rows this step's update leaves unchanged
            const int nmb = p2p_pre_mark_blocks(a);
            RAE_LAUNCH(p, k_p2p_pre, dim3(nmb + p2p_rows_grid(a)), dim3(RAE_BT), 0, st, a, 0, nmb);
        }
    }
    p->t_start = p->t_stop = nullptr;
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

template <int OPT, bool V4, bool BIL>
static void launch_update_b(rae_plan* p, dim3 gu, dim3 bt, hipStream_t st, const StepArgs& a) {
    if constexpr (BIL) {
        // R tensor: k_bil_prep (bf16 operand layout) -> k_bil_rows; then k_update_bil (C / Wb
        // tiles, cost, A / W rows).  Measured at C5 and not kept: a forked stream for the R
        // branch (123 vs 112 us/step: the cross-stream graph edges cost more than the overlap);
        // k_bil_rows with all P fragments in LDS and every load of a tile hoisted into one round
        // trip (29 vs 24 us: two workgroups per CU and the per-workgroup staging cost more).
        if (a.bf16 && !a.fuse_prep) {
            const int gp = 4 * ((a.r + 63) / 64) * (a.Lp / 32) + (a.Lp / 32) * ((a.m + 15) / 16);
            RAE_LAUNCH(p, k_bil_prep, dim3(gp), bt, 0, st, a);
        }
        const int nRt = n_rtiles(a.dec, a.r, a.m);
        const dim3 gr((nRt + RAE_NWAVE - 1) / RAE_NWAVE);
        const size_t lr = bil_rows_lds_bytes(a.m, a.bf16, OPT == 0);
        constexpr size_t lu = 4 * update_lds_floats<V4, 2>();
        if (RAE_BIL_FUSED_UPD && lr >= lu) {
            const dim3 gf(gu.x + gr.x);
            // (PP: the pipelined peer-to-peer form's row pushes compiled in)
            with_bool(a.pipe, [&](auto PP) { with_q(p->q, [&](auto Q) {
                RAE_LAUNCH(p, (k_bil_update<OPT, V4, RAE_CV(Q), RAE_CV(PP)>), gf, bt, lr, st, a, (int)gu.x);
            }); });
            return;
        }
        with_bool(lr != 0, [&](auto LDS) {
            RAE_LAUNCH(p, (k_bil_rows<OPT, RAE_CV(LDS)>), gr, bt, lr, st, a);
        });
        with_bool(a.pipe, [&](auto PP) { with_q(p->q, [&](auto Q) {
            RAE_LAUNCH(p, (k_update_bil<OPT, V4, RAE_CV(Q), RAE_CV(PP)>), gu, bt, 0, st, a);
        }); });
    } else {
        // the data-parallel SP update (wire records: vectors in the vector buffer, dense
        // partials) and the single-rank one are separate instantiations
        with_bool(a.lay.wire != 0, [&](auto WIRE) { with_q(p->q, [&](auto Q) {
            RAE_LAUNCH(p, (k_update<OPT, V4, RAE_CV(Q), RAE_CV(WIRE)>), gu, bt, 0, st, a);
        }); });
    }
}

// k_heavy_fin for the plan's optimizer / vector width / row slots (PP: pipelined pushes)
template <bool PP>
static void launch_heavy_fin(rae_plan* p, dim3 gh, dim3 bt, hipStream_t st, const StepArgs& a) {
    with_opt(a.opt, [&](auto O) { with_bool(p->v4, [&](auto V) { with_q(p->q, [&](auto Q) {
        RAE_LAUNCH(p, (k_heavy_fin<RAE_CV(O), RAE_CV(V), RAE_CV(Q), PP>), gh, bt, 0, st, a);
    }); }); });
}

static int launch_update(rae_plan* p, const int64_t* cursor, int64_t off, hipStream_t st) {
    StepArgs a = p->args;
    a.cursor = cursor;
    a.step_offset = off;
    a.stamps = p->stamps_upd;
    const dim3 gu(p->grid_update), bt(RAE_BT);
    if (p2p_on(p))            // every peer's records of this batch are here
        RAE_LAUNCH(p, k_p2p_wait, dim3(1), dim3(64), 0, st, a, 0, 1u);
    if (a.lay.wire)           // the vectors the wire records left out, for the whole batch
    {
        const dim3 gv(ceil_div(vrec_tasks(a.L, a.r), RAE_NWAVE));
        with_bool(a.m % 4 == 0, [&](auto V) { RAE_LAUNCH(p, k_vrec<RAE_CV(V)>, gv, bt, 0, st, a); });
    }
    with_opt(a.opt, [&](auto O) { with_bool(p->v4, [&](auto V) {
        with_bool(a.dec == RAE_DEC_SP, [&](auto SP) {
            launch_update_b<RAE_CV(O), RAE_CV(V), !RAE_CV(SP)>(p, gu, bt, st, a);
        });
    }); });
    HIPCHK(hipGetLastError());
    if (a.hch) {              // the rows split into chunks: their chunk sums combined + updated
        const dim3 gh(ceil_div(a.HF, RAE_NWAVE));
        with_bool(a.pipe, [&](auto PP) { launch_heavy_fin<RAE_CV(PP)>(p, gh, bt, st, a); });
        HIPCHK(hipGetLastError());
    }
    if (a.reg_on) {
        with_opt(a.opt, [&](auto O) { RAE_LAUNCH(p, k_dense_w<RAE_CV(O)>, dim3(p->grid_dense), bt, 0, st, a); });
        HIPCHK(hipGetLastError());
        RAE_LAUNCH(p, k_finalize_cost, dim3(1), dim3(64), 0, st, a);
        HIPCHK(hipGetLastError());
    }
    if (p2p_on(p) && a.pipe) {   // the next batch's rows are in the peers' replicas
        RAE_LAUNCH(p, k_p2p_signal, dim3(1), dim3(64), 0, st, a, 1);
        HIPCHK(hipGetLastError());
    }
    p->t_start = p->t_stop = nullptr;
    return RAE_OK;
}

static int launch_index(rae_plan* p, int64_t first, int64_t count, hipStream_t st) {
    if (!p->args.neg1 || !p->args.neg2) return fail(RAE_E_STATE, "negatives not set");
    const int64_t nb = p->cfg.n_examples / ((int64_t)p->cfg.batch_size * p->cfg.world_size);
    if (first < 0 || count < 0 || first + count > nb)
        return fail(RAE_E_INVALID, "batch range out of the epoch");
    if (count > p->args.index_window)
        return fail(RAE_E_INVALID, "more batches than the index window holds");
    if (count == 0) return RAE_OK;
    const StepArgs& a = p->args;
    // the slots' partition counts and scatter cursors start at zero (two ranges when the
    // window wraps around the ring)
    {
        const int64_t s0 = first % a.index_window, n0 = std::min(count, a.index_window - s0);
        const size_t per = 4ull * 4 * RAE_IDX_HMAX;
        HIPCHK(hipMemsetAsync(a.gidx + s0 * 4 * RAE_IDX_HMAX, 0, per * n0, st));
        if (count > n0) HIPCHK(hipMemsetAsync(a.gidx, 0, per * (count - n0), st));
    }
    const unsigned nsl = (unsigned)((a.L + RAE_IDX_EPS - 1) / RAE_IDX_EPS);
    const unsigned hmax = (unsigned)(a.HA > a.HW ? a.HA : a.HW);
    hipLaunchKernelGGL(k_idx_count, dim3((unsigned)count, 3, nsl), dim3(RAE_BT), 0, st, a, first);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_idx_scatter, dim3((unsigned)count, 2, nsl), dim3(RAE_BT), 0, st, a, first);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_idx_sort<false>, dim3((unsigned)count, 2, hmax), dim3(RAE_FBT),
                       p->smem_idxf, st, a, first);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_idx_sort<true>, dim3((unsigned)count, 2, hmax), dim3(RAE_FBT),
                       p->smem_idx, st, a, first);
    HIPCHK(hipGetLastError());
    const unsigned ntk = (unsigned)((a.TC + RAE_TASK_PER - 1) / RAE_TASK_PER);
    hipLaunchKernelGGL(k_build_tasks, dim3((unsigned)count, ntk), dim3(RAE_BT), 0, st, a, first);
    HIPCHK(hipGetLastError());
    if (p->args.part) {
        hipLaunchKernelGGL(k_build_dplists, dim3((unsigned)count, p->args.G, 4), dim3(RAE_FBT),
                           4 * RAE_DPL_KEYS + 4 * 32, st, p->args, first);
        HIPCHK(hipGetLastError());
    }
    return RAE_OK;
}

extern "C" int rae_build_index(rae_plan* p, int64_t first, int64_t count, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    return launch_index(p, first, count, (hipStream_t)stream);
}
extern "C" int64_t rae_index_window(rae_plan* p) { return p ? p->args.index_window : -1; }

// read-back of the row index (tests, diagnosis): outside every step path, nothing is written
extern "C" int rae_index_dims(const rae_plan* p, int64_t* out, int32_t count) {
    if (!p || !out) return fail(RAE_E_INVALID, "null argument");
    if (count != RAE_INDEX_NDIMS) return fail(RAE_E_INVALID, "rae_index_dims: count must be RAE_INDEX_NDIMS");
    const StepArgs& a = p->args;
    const int64_t v[RAE_INDEX_NDIMS] = {
        a.L, a.l, a.s, a.G, a.rank, a.part, a.RA, a.RW, a.HA, a.HW, a.index_window, a.posbits,
        a.TC, a.NVC, a.hch, a.HF, a.dcap, a.dstride, a.dnx, a.priv, a.privnf, a.LA, a.LW};
    for (int i = 0; i < RAE_INDEX_NDIMS; ++i) out[i] = v[i];
    return RAE_OK;
}
extern "C" int rae_index_read(rae_plan* p, int64_t batch, int32_t region, void* host_out, int64_t bytes) {
    if (!p || !host_out) return fail(RAE_E_INVALID, "null argument");
    if (batch < 0) return fail(RAE_E_INVALID, "batch index out of the epoch");
    const StepArgs& a = p->args;
    const int64_t slot = batch % a.index_window;
    // (base, bytes per slot) of the region; a null base: the plan has no such region
    const char* base = nullptr;
    int64_t per = 0;
    auto at = [&](const void* ptr, int64_t n) { base = reinterpret_cast<const char*>(ptr); per = n; };
    switch (region) {
    case RAE_IDXR_SREC_A: at(a.srecA, 4ll * a.RA); break;
    case RAE_IDXR_SREC_W: at(a.srecW, 4ll * a.RW); break;
    case RAE_IDXR_SEG_A: at(a.urowA, 16ll * a.RA); break;
    case RAE_IDXR_SEG_W: at(a.urowW, 16ll * a.RW); break;
    case RAE_IDXR_COUNT_A: case RAE_IDXR_COUNT_W:      // gidx[slot][table][0]: the counts
        at(a.gidx, 16ll * RAE_IDX_HMAX);
        if (base) base += (region == RAE_IDXR_COUNT_W ? 8ll : 0ll) * RAE_IDX_HMAX;
        break;
    case RAE_IDXR_PCLS_A: case RAE_IDXR_PCLS_W:
        at(a.pcls, 32ll * RAE_IDX_HMAX);
        if (base) base += (region == RAE_IDXR_PCLS_W ? 16ll : 0ll) * RAE_IDX_HMAX;
        break;
    case RAE_IDXR_THDR: at(a.thdr, 16); break;
    case RAE_IDXR_TASK: at(a.task, 16ll * a.TC); break;
    case RAE_IDXR_VTASK: at(a.vtask, 16ll * a.NVC); break;
    case RAE_IDXR_HFIN: if (a.hch) at(a.hfin, 16ll * a.HF); break;
    case RAE_IDXR_DESC: at(a.desc, 4ll * a.dnx * a.dstride); break;
    case RAE_IDXR_PMASK: if (a.priv) at(a.pmask, 16ll * a.L); break;
    case RAE_IDXR_DPL: if (a.part) at(a.dpl, 4ll * dpl_slot_ints(a.G, a.LA, a.LW)); break;
    case RAE_IDXR_DPC: if (a.part) at(a.dpc, 16ll * a.G); break;
    case RAE_IDXR_DPMAX: if (a.part) at(a.dpmax, 0); break;
    default: return fail(RAE_E_INVALID, "rae_index_read: unknown region");
    }
    if (!base) return fail(RAE_E_INVALID, "rae_index_read: the plan has no such region");
    // what is copied: a slot of the region; the two partition tables one table's
    // RAE_IDX_HMAX entries of the slot; dpmax its two words (not per slot)
    int64_t want = per;
    if (region == RAE_IDXR_COUNT_A || region == RAE_IDXR_COUNT_W) want = 4ll * RAE_IDX_HMAX;
    if (region == RAE_IDXR_PCLS_A || region == RAE_IDXR_PCLS_W) want = 16ll * RAE_IDX_HMAX;
    if (region == RAE_IDXR_DPMAX) want = 8;
    if (bytes != want)
        return fail(RAE_E_INVALID, "rae_index_read: the region holds " + std::to_string(want) + " bytes");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_out, base + slot * per, (size_t)want, hipMemcpyDeviceToHost));
    return RAE_OK;
}

extern "C" int rae_step_forward(rae_plan* p, int64_t off, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    return launch_forward(p, p->d_cursor, off, (hipStream_t)stream);
}
extern "C" int rae_step_update(rae_plan* p, int64_t off, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    return launch_update(p, p->d_cursor, off, (hipStream_t)stream);
}

// absolute-batch forms: the batch index rides in the launch (no device cursor)
static int check_batch(rae_plan* p, int64_t batch) {
    const int64_t nb = p->cfg.n_examples / ((int64_t)p->cfg.batch_size * p->cfg.world_size);
    if (batch < 0 || batch >= nb) return fail(RAE_E_INVALID, "batch index out of the epoch");
    return RAE_OK;
}
extern "C" int rae_step_forward_at(rae_plan* p, int64_t batch, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (int rc = check_batch(p, batch)) return rc;
    return launch_forward(p, nullptr, batch, (hipStream_t)stream);
}
extern "C" int rae_step_update_at(rae_plan* p, int64_t batch, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (int rc = check_batch(p, batch)) return rc;
    return launch_update(p, nullptr, batch, (hipStream_t)stream);
}

// ---- partitioned data-parallel update (rae_dp.hpp) ----
extern "C" int64_t rae_dp_block_floats(const rae_config* cfg, int32_t cap_entities,
                                       int32_t cap_features) {
    if (!cfg || cap_entities < 0 || cap_features < 0) return -1;
    return dp_block_floats(cfg->embed, cfg->relations, cap_entities, cap_features);
}
extern "C" int rae_set_dp_buffers(rae_plan* p, float* send, float* recv, int32_t cap_entities,
                                  int32_t cap_features) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (!p->args.part) return fail(RAE_E_STATE, "the plan's data-parallel update is not partitioned");
    if ((p->args.xchg == RAE_XCHG_COLLECTIVE && (!send || !recv)) || cap_entities < 0 || cap_features < 0 ||
        cap_entities > p->args.LA || cap_features > p->args.LW)
        return fail(RAE_E_INVALID, "bad row-exchange buffers / capacities");
    StepArgs& a = p->args;
    a.dsend = send;
    a.drecv = recv;
    a.capA = cap_entities;
    a.capW = cap_features;
    a.dblk = dp_block_floats(a.r, a.m, a.capA, a.capW);
    return RAE_OK;
}
extern "C" int rae_dp_list_max(rae_plan* p, int32_t* max_entities, int32_t* max_features) {
    if (!p || !max_entities || !max_features) return fail(RAE_E_INVALID, "null argument");
    int v[2] = {0, 0};
    HIPCHK(hipMemcpy(v, p->args.dpmax, sizeof(v), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(p->args.dpmax, 0, sizeof(v)));
    *max_entities = v[0];
    *max_features = v[1];
    return RAE_OK;
}
static int launch_dp_move(rae_plan* p, bool pack, const int64_t* cursor, int64_t off, hipStream_t st) {
    const StepArgs& a0 = p->args;
    if (!a0.part) return fail(RAE_E_STATE, "the plan's data-parallel update is not partitioned");
    if (a0.G == 1) return RAE_OK;                   // every row is this rank's
    if (!a0.dsend || !a0.drecv) return fail(RAE_E_STATE, "row-exchange buffers not set (the "
                                                       "peer-to-peer exchange has none: its rows "
                                                       "move inside rae_step_forward)");
    StepArgs a = a0;
    a.cursor = cursor;
    a.step_offset = off;
    const int64_t waves = (int64_t)a.G * (a.capA + a.capW);
    if (waves == 0) return RAE_OK;
    const dim3 gr((unsigned)((waves + RAE_NWAVE - 1) / RAE_NWAVE));
    with_bool(pack, [&](auto PACK) { RAE_LAUNCH(p, k_dp_move<RAE_CV(PACK)>, gr, dim3(RAE_BT), 0, st, a); });
    p->t_start = p->t_stop = nullptr;
    HIPCHK(hipGetLastError());
    return RAE_OK;
}
extern "C" int rae_dp_pack(rae_plan* p, int64_t off, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    return launch_dp_move(p, true, p->d_cursor, off, (hipStream_t)stream);
}
extern "C" int rae_dp_unpack(rae_plan* p, int64_t off, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    return launch_dp_move(p, false, p->d_cursor, off, (hipStream_t)stream);
}
extern "C" int rae_dp_pack_at(rae_plan* p, int64_t batch, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (int rc = check_batch(p, batch)) return rc;
    return launch_dp_move(p, true, nullptr, batch, (hipStream_t)stream);
}
extern "C" int rae_dp_unpack_at(rae_plan* p, int64_t batch, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (int rc = check_batch(p, batch)) return rc;
    return launch_dp_move(p, false, nullptr, batch, (hipStream_t)stream);
}

// ---- peer-to-peer exchange (rae_p2p.hpp) ----
extern "C" int rae_ipc_export(const void* ptr, void* handle_out, int64_t* offset_out) {
    if (!ptr || !handle_out || !offset_out) return fail(RAE_E_INVALID, "null argument");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    HIPCHK(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr));
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, (void*)base));
    static_assert(sizeof(h) == RAE_IPC_HANDLE_BYTES, "IPC handle size");
    memcpy(handle_out, &h, sizeof(h));
    *offset_out = (int64_t)((const char*)ptr - (const char*)base);
    return RAE_OK;
}
extern "C" int rae_ipc_open(const void* handle, void** base_out) {
    if (!handle || !base_out) return fail(RAE_E_INVALID, "null argument");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    HIPCHK(hipIpcOpenMemHandle(base_out, h, hipIpcMemLazyEnablePeerAccess));
    return RAE_OK;
}
extern "C" int rae_ipc_close(void* base) {
    if (!base) return fail(RAE_E_INVALID, "null argument");
    HIPCHK(hipIpcCloseMemHandle(base));
    return RAE_OK;
}
extern "C" void* rae_p2p_signals(rae_plan* p) { return p ? (void*)p->d_sig : nullptr; }
extern "C" int rae_set_peer(rae_plan* p, int32_t peer, float* exchange, float* W, float* A,
                            float* Ab, void* signals) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (p->args.xchg == RAE_XCHG_COLLECTIVE) return fail(RAE_E_STATE, "the plan's exchange is not peer-to-peer");
    if (peer < 0 || peer >= p->args.G || peer == p->args.rank)
        return fail(RAE_E_INVALID, "peer must be another rank");
    if (!exchange || !W || !A || !Ab || !signals) return fail(RAE_E_INVALID, "null peer buffer");
    const PeerBufs pb{exchange, W, A, Ab, (unsigned*)signals};
    HIPCHK(hipMemcpy(p->args.peers + peer, &pb, sizeof(pb), hipMemcpyHostToDevice));
    p->peers_mask |= 1 << peer;
    p->peers_set = p->peers_mask == (((1 << p->args.G) - 1) & ~(1 << p->args.rank));
    return RAE_OK;
}
extern "C" int rae_p2p_prologue(rae_plan* p, int64_t batch, int32_t drain, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (!p2p_on(p) || !p->args.pipe)
        return fail(RAE_E_STATE, "the plan's exchange is not the pipelined peer-to-peer form");
    if (!p->peers_set) return fail(RAE_E_STATE, "peer buffers not set (rae_set_peer)");
    if (int rc = check_batch(p, batch)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    StepArgs a = p->args;
    a.cursor = nullptr;
    a.step_offset = batch;
    if (drain)                // the signal of rows a previous step pushed for another batch
        RAE_LAUNCH(p, k_p2p_wait, dim3(1), dim3(64), 0, st, a, 1, 1u);
    HIPCHK(hipMemsetAsync(a.pm, 0, 4ull * 2 * (a.pmA + a.pmW), st));
    const int nmb = p2p_pre_mark_blocks(a);
    RAE_LAUNCH(p, k_p2p_pre, dim3(nmb + p2p_rows_grid(a)), dim3(RAE_BT), 0, st, a, 1, nmb);
    RAE_LAUNCH(p, k_p2p_signal, dim3(1), dim3(64), 0, st, a, 1);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}
extern "C" int rae_set_p2p_timeout(rae_plan* p, double seconds) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (p->args.xchg == RAE_XCHG_COLLECTIVE) return fail(RAE_E_STATE, "the plan's exchange is not peer-to-peer");
    if (!(seconds > 0.0) || seconds > 3600.0) return fail(RAE_E_INVALID, "timeout must be in (0, 3600] s");
    p->args.p2p_timeout = (unsigned long long)(seconds * 1e8);   // s_memrealtime: 100 MHz
    return RAE_OK;
}

extern "C" int rae_time_next(rae_plan* p, void* start, void* stop) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (!start || !stop) return fail(RAE_E_INVALID, "null event");
    p->t_start = (hipEvent_t)start;
    p->t_stop = (hipEvent_t)stop;
    return RAE_OK;
}
extern "C" int rae_event_create(void** ev) {
    if (!ev) return fail(RAE_E_INVALID, "null argument");
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    *ev = (void*)e;
    return RAE_OK;
}
extern "C" int rae_event_destroy(void* ev) {
    if (ev) HIPCHK(hipEventDestroy((hipEvent_t)ev));
    return RAE_OK;
}
extern "C" int rae_event_elapsed_ms(void* start, void* stop, float* ms) {
    if (!start || !stop || !ms) return fail(RAE_E_INVALID, "null argument");
    HIPCHK(hipEventSynchronize((hipEvent_t)stop));
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return RAE_OK;
}

extern "C" int rae_train_step(rae_plan* p, int64_t batch, const int32_t* n1, const int32_t* n2,
                              rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    if (p->cfg.world_size != 1)
        return fail(RAE_E_STATE, "rae_train_step is the single-rank func['train'] path");
    const int64_t nb = p->cfg.n_examples / p->cfg.batch_size;
    if (batch < 0 || batch >= nb) return fail(RAE_E_INVALID, "batch index out of range");
    int rc = rae_set_negatives(p, n1, n2, RAE_NEG_PER_CALL, p->cfg.batch_size);
    if (rc) return rc;
    rc = launch_index(p, batch, 1, (hipStream_t)stream);
    if (rc) return rc;
    rc = launch_forward(p, nullptr, batch, (hipStream_t)stream);
    if (rc) return rc;
    return launch_update(p, nullptr, batch, (hipStream_t)stream);
}

#ifdef RAE_STAMPS
// diagnostic build only: point the kernels at a stamp buffer (16 u64 per forward block,
// 4 u64 per update wave); fwd=1 -> forward launches, fwd=0 -> update launches
extern "C" int rae_debug_stamps(rae_plan* p, unsigned long long* buf, int fwd) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    p->stamps_fwd = fwd ? buf : nullptr;
    p->stamps_upd = fwd ? nullptr : buf;
    return RAE_OK;
}
extern "C" int rae_debug_grid(rae_plan* p, int* out) {
    out[0] = p->grid_fwd; out[1] = p->grid_update; out[2] = 0; out[3] = 0;
    return RAE_OK;
}
#ifdef RAE_WSTAMPS
// the fast SP forward's per-wave stamps (tools/c_stream_stamps.py): a buffer of their own, 8 u64
// per wave = 64 per forward block, so a library built with them stays safe under the tools that
// pass rae_debug_stamps' 16 u64 per block (null: no wave stamps are written)
extern "C" int rae_debug_wave_stamps(rae_plan* p, unsigned long long* buf) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    p->stamps_wave = buf;
    return RAE_OK;
}
#endif
#endif

// the device error word, bit by bit (rae.h): a peer-to-peer wait timeout is a state error (a
// peer stopped signalling), everything else a capacity overflow
static int err_flags(int e) {
    if (!e) return RAE_OK;
    static const struct { int bit; const char* what; } bits[] = {
        {1, "an entity-row index partition overflowed its LDS sort"},
        {2, "a feature-row index partition overflowed its LDS sort"},
        {4, "a batch exceeded the row index's record capacity"},
        {8, "a data-parallel row list overflowed while being built"},
        {16, "a data-parallel row list is longer than the exchange's row capacity"},
        {64, "a peer-to-peer wait timed out (a peer stopped signalling)"},
    };
    std::string msg;
    for (const auto& b : bits)
        if (e & b.bit) msg += (msg.empty() ? "" : "; ") + std::string(b.what);
    msg += " (device error flags=" + std::to_string(e) + ")";
    return fail(e & 64 ? RAE_E_STATE : RAE_E_OVERFLOW, msg);
}
extern "C" int rae_check(rae_plan* p) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    int e = 0;
    HIPCHK(hipMemcpy(&e, p->d_err, sizeof(int), hipMemcpyDeviceToHost));
    return err_flags(e);
}
// the same read ordered on one stream (pinned host word): the caller waits for that stream's
// queued work only
extern "C" int rae_check_on(rae_plan* p, rae_stream_t stream) {
    if (!p) return fail(RAE_E_INVALID, "null plan");
    HIPCHK(hipMemcpyAsync(p->h_err, p->d_err, sizeof(int), hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return err_flags(*p->h_err);
}

static int launch_neg(const double* cum, int64_t n, const double* u, uint64_t seed,
                      uint64_t offset, int64_t count, int32_t* out, hipStream_t st, bool philox) {
    if (!cum || !out || (!philox && !u)) return fail(RAE_E_INVALID, "null argument");
    if (n < 1 || n >= (1ll << 31)) return fail(RAE_E_INVALID, "CDF size must be in [1, 2^31)");
    if (count <= 0) return RAE_OK;
    int64_t blocks = (count + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (philox)
        hipLaunchKernelGGL(k_neg_sample<true>, dim3((unsigned)blocks), dim3(256), 0, st, cum, n, u,
                           seed, offset, count, out);
    else
        hipLaunchKernelGGL(k_neg_sample<false>, dim3((unsigned)blocks), dim3(256), 0, st, cum, n, u,
                           seed, offset, count, out);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

extern "C" int rae_neg_sample(const double* cum, int64_t n, const double* u, int64_t count,
                              int32_t* out, rae_stream_t stream) {
    return launch_neg(cum, n, u, 0, 0, count, out, (hipStream_t)stream, false);
}
extern "C" int rae_neg_sample_philox(const double* cum, int64_t n, uint64_t seed, uint64_t offset,
                                     int64_t count, int32_t* out, rae_stream_t stream) {
    return launch_neg(cum, n, nullptr, seed, offset, count, out, (hipStream_t)stream, true);
}

extern "C" int rae_stream_copy(const void* src, void* dst, int64_t bytes, rae_stream_t stream) {
    if (!src || !dst) return fail(RAE_E_INVALID, "null argument");
    if (bytes < 0 || (bytes & 15) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
        return fail(RAE_E_INVALID, "bytes and pointers must be multiples of 16");
    const int64_t n = bytes / 16;
    if (n == 0) return RAE_OK;
    int64_t grid = (n + 1023) / 1024;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(k_stream_copy, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                       (const rae_v4f*)src, (rae_v4f*)dst, n);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

extern "C" int rae_mfma_probe(int64_t iters, int32_t blocks, float* sink, rae_stream_t stream) {
    if (!sink || iters < 1 || blocks < 1) return fail(RAE_E_INVALID, "bad argument");
    hipLaunchKernelGGL(k_mfma_probe, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       iters, sink);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

extern "C" int rae_label(const int32_t* indptr, const int32_t* indices, const float* values,
                         const float* W, const float* Wb, int32_t m, int64_t row0, int64_t nrows,
                         int64_t* labels, float* probs, rae_stream_t stream) {
    if (!indptr || !indices || !W || !Wb || !labels) return fail(RAE_E_INVALID, "null argument");
    if (m < 1 || m > 512) return fail(RAE_E_INVALID, "relations must be in [1, 512] for labelling");
    const bool v4 = (m % 4) == 0;
    if (!v4 && m > 128)
        return fail(RAE_E_INVALID, "relations must be a multiple of 4 above 128 for labelling");
    if (nrows <= 0) return RAE_OK;
    int64_t blocks = (nrows + RAE_NWAVE - 1) / RAE_NWAVE;
    if (blocks > 65536) blocks = 65536;
    if (v4)
        hipLaunchKernelGGL(k_label<true>, dim3((unsigned)blocks), dim3(RAE_BT), 0, (hipStream_t)stream,
                           indptr, indices, values, W, Wb, m, row0, nrows, labels, probs);
    else
        hipLaunchKernelGGL(k_label<false>, dim3((unsigned)blocks), dim3(RAE_BT), 0, (hipStream_t)stream,
                           indptr, indices, values, W, Wb, m, row0, nrows, labels, probs);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

// ---- plan-free evaluation: the argument checks, workspace blocks and launch prelude that
// ---- rae_eval_cost / _rank / _topk / _relations share (host only) -----------------------------
namespace {
inline size_t ev_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the argument checks the entries share; each fails with the text its entry always had
int count_range(const char* name, int64_t v, int64_t lo) {    // lo <= v < 2^31
    if (v < lo || v >= (1ll << 31))
        return fail(RAE_E_INVALID, std::string(name) + " must be in [" + std::to_string(lo) + ", 2^31)");
    return RAE_OK;
}
int entity_count(int64_t n) { return count_range("n_entities", n, 1); }
int relations_range(int m) {
    if (m < 1 || m > 512) return fail(RAE_E_INVALID, "relations must be in [1, 512]");
    return RAE_OK;
}
int key_count(int n_keys) {
    if (n_keys < 1 || n_keys > (1 << 22)) return fail(RAE_E_INVALID, "n_keys must be in [1, 2^22]");
    return RAE_OK;
}
struct NamedPtr { const void* p; const char* name; };
int not_null(std::initializer_list<NamedPtr> ps) {            // the first NULL one, in list order
    for (const NamedPtr& n : ps)
        if (!n.p) return fail(RAE_E_INVALID, std::string(n.name) + " is NULL");
    return RAE_OK;
}
int aligned(std::initializer_list<const void*> ps, uintptr_t mask, const char* msg) {
    for (const void* p : ps)
        if ((uintptr_t)p & mask) return fail(RAE_E_INVALID, msg);
    return RAE_OK;
}
// shapes of the caller-given-queries entries (rae_rank_queries, rae_topk_queries)
int query_shapes(int embed, int64_t n_entities) {
    if (embed < 1 || embed > 1024) return fail(RAE_E_INVALID, "embed must be in [1, 1024]");
    return entity_count(n_entities);
}
// the shape limits of the evaluation kernels, in two halves (eval_shapes checks neg_samples
// between them)
int model_shapes(int dec, int m, int r) {
    if (dec < 0 || dec > 2) return fail(RAE_E_INVALID, "decoder must be 0..2");
    if (const int rc = relations_range(m)) return rc;
    if ((m % 4) != 0 && m > 128)
        return fail(RAE_E_INVALID, "relations must be a multiple of 4 above 128");
    if (r < 1 || r > 1024) return fail(RAE_E_INVALID, "embed must be in [1, 1024]");
    return RAE_OK;
}
int bilinear_shapes(int dec, int m) {
    if (dec != RAE_DEC_SP && eval_mt_lds_bytes(m) > 160 * 1024)
        return fail(RAE_E_INVALID, "relations must be <= 320 for the bilinear decoders");
    return RAE_OK;
}
int eval_shapes(const rae_eval_args* a, bool need_s) {
    if (!a) return fail(RAE_E_INVALID, "null argument");
    if (const int rc = model_shapes(a->decoder, a->relations, a->embed)) return rc;
    if (need_s && a->neg_samples < 1) return fail(RAE_E_INVALID, "neg_samples must be >= 1");
    if (const int rc = bilinear_shapes(a->decoder, a->relations)) return rc;
    if (eval_dec_lds_floats(a->decoder, a->relations, a->embed) * 4 > 160 * 1024)
        return fail(RAE_E_INVALID, "relations / embed need more than 160 KiB of LDS per tile");
    return RAE_OK;
}
// the shapes of the relation-score kernel: the same limits without the tile's
int rel_shapes(int dec, int m, int r, int64_t n_entities) {
    if (const int rc = model_shapes(dec, m, r)) return rc;
    if (const int rc = bilinear_shapes(dec, m)) return rc;
    return entity_count(n_entities);
}

// the buffer check of the four entries, in blocks: each entry calls them in this order with its
// own outputs' checks between them
int check_rows(const rae_eval_args* a) {
    if (a->nrows < 0) return fail(RAE_E_INVALID, "nrows must be >= 0");
    if (a->row0 < 0 || a->row0 + a->nrows >= (1ll << 31))
        return fail(RAE_E_INVALID, "row0 / nrows out of range");
    return RAE_OK;
}
int check_model(const rae_eval_args* a) {
    if (!a->W) return fail(RAE_E_INVALID, "W is NULL");
    if (!a->Wb) return fail(RAE_E_INVALID, "Wb is NULL");
    if (!a->A) return fail(RAE_E_INVALID, "A is NULL");
    if (!a->Ab) return fail(RAE_E_INVALID, "Ab is NULL");
    if (a->decoder != RAE_DEC_RESCAL && (!a->C1 || !a->C2))
        return fail(RAE_E_INVALID, "C1 / C2 is NULL");
    if (a->decoder != RAE_DEC_SP && !a->R3) return fail(RAE_E_INVALID, "R3 is NULL");
    if (!a->indptr || !a->indices) return fail(RAE_E_INVALID, "indptr / indices is NULL");
    if (!a->args1 || !a->args2) return fail(RAE_E_INVALID, "args1 / args2 is NULL");
    return RAE_OK;
}
int check_workspace(const void* ws, int64_t bytes, size_t need, const char* sizer) {
    if (!ws) return fail(RAE_E_INVALID, "workspace is NULL");
    if ((uintptr_t)ws & 255) return fail(RAE_E_INVALID, "workspace must be 256-byte aligned");
    if (bytes < (int64_t)need)
        return fail(RAE_E_INVALID, std::string("workspace_bytes is smaller than ") + sizer + "()");
    return RAE_OK;
}
int check_align(const rae_eval_args* a) {
    if ((a->relations % 4) == 0 && (((uintptr_t)a->W | (uintptr_t)a->Wb | (uintptr_t)a->C1 |
                                     (uintptr_t)a->C2 | (uintptr_t)a->R3) & 15))
        return fail(RAE_E_INVALID, "W / Wb / C1 / C2 / R3 must be 16-byte aligned");
    if ((a->embed % 4) == 0 && ((uintptr_t)a->A & 15))
        return fail(RAE_E_INVALID, "A must be 16-byte aligned");
    return RAE_OK;
}

// workspace blocks, laid from offset o on; each returns the offset past its block
struct EncWs { size_t o_terms, o_P, o_v, o_w; };      // the encoder prelude's, of ch examples
struct QueryWs { size_t o_Q, o_c, o_u, o_skip; };     // the 2 ch queries k_rank_build writes
size_t lay_enc(const rae_eval_args* a, size_t ch, size_t o, EncWs& L) {
    const bool bil = a->decoder != RAE_DEC_SP;
    const size_t m = (size_t)a->relations, r4 = (size_t)eval_r4(a->embed);
    L.o_terms = o;   o = ev_align(o + ch * 3 * sizeof(float));
    L.o_P = o;       if (bil) o = ev_align(o + ch * m * sizeof(float));
    L.o_v = o;       if (bil) o = ev_align(o + (size_t)eval_nbj(a->embed) * ch * r4 * sizeof(float));
    L.o_w = o;       if (bil) o = ev_align(o + (size_t)eval_nbi(a->embed) * ch * r4 * sizeof(float));
    return o;
}
size_t lay_queries(const rae_eval_args* a, size_t ch, size_t o, QueryWs& L) {
    L.o_Q = o;       o = ev_align(o + 2 * ch * (size_t)eval_r4(a->embed) * sizeof(float));
    L.o_c = o;       o = ev_align(o + 2 * ch * sizeof(float));
    L.o_u = o;       o = ev_align(o + 2 * ch * sizeof(float));
    L.o_skip = o;    o = ev_align(o + 2 * ch * sizeof(int32_t));
    return o;
}

// the kernels' arguments of chunks of cap examples, without negatives (rae_eval_cost adds them);
// row0 and n are the chunk's
EvalArgs eval_args_of(const rae_eval_args* a, int cap, const EncWs& L) {
    char* ws = (char*)a->workspace;
    EvalArgs e;
    e.dec = a->decoder; e.m = a->relations; e.r = a->embed; e.s = 0; e.alpha = a->alpha;
    e.W = a->W; e.Wb = a->Wb; e.A = a->A; e.Ab = a->Ab; e.C1 = a->C1; e.C2 = a->C2; e.R3 = a->R3;
    e.indptr = a->indptr; e.indices = a->indices; e.values = a->values;
    e.args1 = a->args1; e.args2 = a->args2; e.neg1 = nullptr; e.neg2 = nullptr;
    e.neg_stride = 0;
    e.cap = cap; e.r4 = eval_r4(a->embed);
    e.terms = (float*)(ws + L.o_terms);
    e.P = (float*)(ws + L.o_P); e.vpart = (float*)(ws + L.o_v); e.wpart = (float*)(ws + L.o_w);
    return e;
}
// large dynamic LDS is opted into per kernel (not a stream operation): the decoder-side kernel
// of the entry and k_eval_mt
int eval_large_lds(const void* dec_kernel, const rae_eval_args* a) {
    const size_t lds_dec = eval_dec_lds_floats(a->decoder, a->relations, a->embed) * 4;
    const size_t lds_mt = eval_mt_lds_bytes(a->relations);
    const bool v4 = (a->relations % 4) == 0;
    if (lds_dec > 48 * 1024)
        HIPCHK(hipFuncSetAttribute(dec_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_dec));
    if (a->decoder != RAE_DEC_SP && lds_mt > 48 * 1024)
        HIPCHK(hipFuncSetAttribute(v4 ? (const void*)k_eval_mt<true> : (const void*)k_eval_mt<false>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_mt));
    return RAE_OK;
}
// the bilinear decoders' prelude of one chunk: P and the partials of M a2 / M^T a1
void launch_enc_mt(const EvalArgs& e, hipStream_t st) {
    if (e.dec == RAE_DEC_SP) return;
    const dim3 ge((unsigned)std::min(ceil_div(e.n, RAE_EV_NW), 65536));
    const dim3 gm((unsigned)(eval_nbi(e.r) * eval_nbj(e.r)));
    with_bool((e.m % 4) == 0, [&](auto V) {
        hipLaunchKernelGGL(k_eval_enc<RAE_CV(V)>, ge, dim3(RAE_EV_BT), 0, st, e);
        hipLaunchKernelGGL(k_eval_mt<RAE_CV(V)>, gm, dim3(RAE_EV_MTT), eval_mt_lds_bytes(e.m), st, e);
    });
}
}  // namespace

// ---- forward-only objective -----------------------------------------------------------------
namespace {
struct EvalLayout {
    int64_t chunk;                           // examples per launch round
    size_t o_partial, total;
    EncWs enc;
};
int eval_layout(const rae_eval_args* a, EvalLayout& L) {
    if (const int rc = eval_shapes(a, true)) return rc;
    L.chunk = a->decoder != RAE_DEC_SP ? RAE_EV_CHUNK_BIL : RAE_EV_CHUNK_SP;
    const size_t ch = (size_t)L.chunk;
    L.o_partial = 0;
    L.total = lay_enc(a, ch, ev_align((ch / RAE_EV_SUMROWS) * 3 * sizeof(double)), L.enc);
    return RAE_OK;
}
}  // namespace

extern "C" int64_t rae_eval_workspace_bytes(const rae_eval_args* a) {
    EvalLayout L;
    if (eval_layout(a, L)) return -1;
    return (int64_t)L.total;
}

extern "C" int rae_eval_cost(const rae_eval_args* a, rae_stream_t stream) {
    EvalLayout L;
    if (const int rc = eval_layout(a, L)) return rc;
    if (const int rc = entity_count(a->n_entities)) return rc;
    if (const int rc = check_rows(a)) return rc;
    if (const int rc = check_model(a)) return rc;
    if (!a->neg1 || !a->neg2) return fail(RAE_E_INVALID, "neg1 / neg2 is NULL");
    if (a->neg_stride < a->row0 + a->nrows)
        return fail(RAE_E_INVALID, "neg_stride is smaller than row0 + nrows");
    if (!a->sums_out) return fail(RAE_E_INVALID, "sums_out is NULL");
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes, L.total,
                                       "rae_eval_workspace_bytes"))
        return rc;
    if (const int rc = check_align(a)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = (a->relations % 4) == 0;
    double* partial = (double*)((char*)a->workspace + L.o_partial);
    const size_t lds_dec = eval_dec_lds_floats(a->decoder, a->relations, a->embed) * 4;
    if (const int rc = eval_large_lds(
            v4 ? (const void*)k_eval_dec<true> : (const void*)k_eval_dec<false>, a))
        return rc;
    EvalArgs e = eval_args_of(a, (int)L.chunk, L.enc);
    e.s = a->neg_samples; e.neg1 = a->neg1; e.neg2 = a->neg2; e.neg_stride = a->neg_stride;
    float* const terms = e.terms;
    if (a->nrows == 0) {
        hipLaunchKernelGGL(k_eval_acc, dim3(1), dim3(64), 0, st, partial, 0, a->sums_out, 1);
        HIPCHK(hipGetLastError());
        return RAE_OK;
    }
    for (int64_t c0 = 0; c0 < a->nrows; c0 += L.chunk) {
        const int n = (int)std::min<int64_t>(L.chunk, a->nrows - c0);
        e.row0 = a->row0 + c0;
        e.n = n;
        e.terms = a->terms_out ? a->terms_out + c0 * 3 : terms;
        launch_enc_mt(e, st);
        const dim3 gd((unsigned)ceil_div(n, RAE_EV_TE));
        with_bool(v4, [&](auto V) {
            hipLaunchKernelGGL(k_eval_dec<RAE_CV(V)>, gd, dim3(RAE_EV_BT), lds_dec, st, e);
        });
        const int nblk = ceil_div(n, RAE_EV_SUMROWS);
        hipLaunchKernelGGL(k_eval_blocksum, dim3((unsigned)nblk), dim3(RAE_EV_BT), 0, st,
                           (const float*)e.terms, n, partial);
        hipLaunchKernelGGL(k_eval_acc, dim3(1), dim3(64), 0, st, (const double*)partial, nblk,
                           a->sums_out, c0 == 0 ? 1 : 0);
        HIPCHK(hipGetLastError());
    }
    return RAE_OK;
}

// ---- argument ranking over all entities -------------------------------------------------------
namespace {
struct RankLayout {                          // rae_eval_rank's workspace
    size_t o_partial, o_lse, o_part, total;
    EncWs enc;
    QueryWs q;
};
inline size_t rank_part_bytes(int64_t n) {
    return ev_align((size_t)rank_strips(n) * RAE_RK_QCHUNK * sizeof(float2));
}
// shapes of rae_eval_rank and its workspace layout (host only)
int eval_rank_layout(const rae_eval_args* a, RankLayout& L) {
    if (const int rc = eval_shapes(a, false)) return rc;
    if (const int rc = entity_count(a->n_entities)) return rc;
    const size_t ch = RAE_RK_ROWCHUNK;
    L.o_partial = 0;
    size_t o = ev_align((ch / RAE_EV_SUMROWS) * RAE_RK_NSUM * sizeof(double));
    o = lay_queries(a, ch, lay_enc(a, ch, o, L.enc), L.q);
    L.o_lse = o;     o = ev_align(o + 2 * ch * sizeof(float));
    L.o_part = o;    o += rank_part_bytes(a->n_entities);
    L.total = o;
    return RAE_OK;
}
// the rank / top-k prelude of one chunk e of RAE_RK_ROWCHUNK rows: its 2 e.n queries built on the
// stream, and the arguments that rank them (u: where the true entities' scores go, or the
// workspace's)
RankArgs rank_queries_of(const EvalArgs& e, const rae_eval_args* a, const QueryWs& L, float* u,
                         hipStream_t st) {
    char* ws = (char*)a->workspace;
    RankBuild b;
    b.Q = (float*)(ws + L.o_Q);
    b.c = (float*)(ws + L.o_c);
    b.u = u ? u : (float*)(ws + L.o_u);
    b.skip = (int32_t*)(ws + L.o_skip);
    const dim3 gd((unsigned)ceil_div(e.n, RAE_EV_TE));
    const size_t lds_dec = eval_dec_lds_floats(e.dec, e.m, e.r) * 4;
    with_bool((e.m % 4) == 0, [&](auto V) {
        hipLaunchKernelGGL(k_rank_build<RAE_CV(V)>, gd, dim3(RAE_EV_BT), lds_dec, st, e, b);
    });
    RankArgs k;
    k.Q = b.Q; k.ldq = e.r4; k.add = b.c; k.target = b.u; k.skip = b.skip;
    k.A = a->A; k.Ab = a->Ab; k.n = a->n_entities; k.r = e.r; k.nq = 2 * e.n;
    return k;
}
// one chunk (k.nq <= RAE_RK_QCHUNK queries) on the stream: zero, scores, the lse's finish
void rank_launch(RankArgs k, float* lse, hipStream_t st) {
    const int strips = rank_strips(k.n);
    k.tps = rank_tiles_per_strip(k.n);
    k.ntiles = rank_tiles(k.n);
    const bool av4 = (k.r % 4) == 0;
    hipLaunchKernelGGL(k_rank_zero, dim3((unsigned)ceil_div(k.nq, 256)), dim3(256), 0, st,
                       k.greater, k.equal, k.nq);
    const dim3 grid((unsigned)ceil_div(k.nq, RAE_RK_TQ), (unsigned)strips);
    with_bool(av4, [&](auto V) {
        with_bool(lse != nullptr, [&](auto L) {
            hipLaunchKernelGGL((k_rank<RAE_CV(V), RAE_CV(L)>), grid, dim3(RAE_RK_BT), 0, st, k);
        });
    });
    if (lse)
        hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)ceil_div(k.nq, 256)), dim3(256), 0, st,
                           (const float2*)k.part, strips, k.nq, lse);
}
}  // namespace

extern "C" int64_t rae_rank_workspace_bytes(const rae_rank_args* q, const rae_eval_args* e) {
    if ((q != nullptr) == (e != nullptr))
        return fail(RAE_E_INVALID, "give exactly one of the two argument structs"), -1;
    if (q) {
        if (query_shapes(q->embed, q->n_entities)) return -1;
        return (int64_t)rank_part_bytes(q->n_entities);
    }
    RankLayout L;
    if (eval_rank_layout(e, L)) return -1;
    return (int64_t)L.total;
}

extern "C" int rae_rank_queries(const rae_rank_args* a, rae_stream_t stream) {
    if (!a) return fail(RAE_E_INVALID, "null argument");
    if (const int rc = query_shapes(a->embed, a->n_entities)) return rc;
    if (a->nq < 0) return fail(RAE_E_INVALID, "nq must be >= 0");
    if (a->ldq < a->embed) return fail(RAE_E_INVALID, "ldq is smaller than embed");
    if (a->ldq % 4) return fail(RAE_E_INVALID, "ldq must be a multiple of 4");
    if (a->nq == 0) return RAE_OK;            // nothing is read or written
    if (!a->Q) return fail(RAE_E_INVALID, "Q is NULL");
    if ((uintptr_t)a->Q & 15) return fail(RAE_E_INVALID, "Q must be 16-byte aligned");
    if (!a->target) return fail(RAE_E_INVALID, "target is NULL");
    if (!a->A) return fail(RAE_E_INVALID, "A is NULL");
    if ((a->embed % 4) == 0 && ((uintptr_t)a->A & 15))
        return fail(RAE_E_INVALID, "A must be 16-byte aligned");
    if (!a->greater || !a->equal) return fail(RAE_E_INVALID, "greater / equal is NULL");
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes,
                                       rank_part_bytes(a->n_entities), "rae_rank_workspace_bytes"))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    for (int64_t c0 = 0; c0 < a->nq; c0 += RAE_RK_QCHUNK) {
        RankArgs k;
        k.Q = a->Q + c0 * a->ldq; k.ldq = a->ldq;
        k.add = a->add ? a->add + c0 : nullptr;
        k.target = a->target + c0;
        k.skip = a->skip ? a->skip + c0 : nullptr;
        k.A = a->A; k.Ab = a->Ab; k.n = a->n_entities; k.r = a->embed;
        k.nq = (int)std::min<int64_t>(RAE_RK_QCHUNK, a->nq - c0);
        k.greater = a->greater + c0; k.equal = a->equal + c0;
        k.part = (float2*)a->workspace;
        rank_launch(k, a->lse ? a->lse + c0 : nullptr, st);
        HIPCHK(hipGetLastError());
    }
    return RAE_OK;
}

extern "C" int rae_eval_rank(const rae_eval_args* a, const rae_rank_out* out, rae_stream_t stream) {
    RankLayout L;
    if (const int rc = eval_rank_layout(a, L)) return rc;
    if (!out) return fail(RAE_E_INVALID, "out is NULL");
    if (const int rc = check_rows(a)) return rc;
    if (const int rc = check_model(a)) return rc;
    if (a->nrows > 0 && (!out->greater || !out->equal))
        return fail(RAE_E_INVALID, "greater / equal is NULL");
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes, L.total,
                                       "rae_rank_workspace_bytes"))
        return rc;
    if (const int rc = check_align(a)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)a->workspace;
    double* partial = (double*)(ws + L.o_partial);
    if (const int rc = eval_large_lds((a->relations % 4) == 0 ? (const void*)k_rank_build<true>
                                                               : (const void*)k_rank_build<false>, a))
        return rc;
    EvalArgs e = eval_args_of(a, RAE_RK_ROWCHUNK, L.enc);
    const bool want_lse = out->lse || out->summary;
    RankHits hk;
    for (int j = 0; j < 4; ++j) hk.k[j] = out->hits_k[j];
    if (a->nrows == 0) {
        if (out->summary) {
            hipLaunchKernelGGL(k_rank_acc, dim3(1), dim3(64), 0, st, (const double*)partial, 0,
                               out->summary, 1);
            HIPCHK(hipGetLastError());
        }
        return RAE_OK;
    }
    for (int64_t c0 = 0; c0 < a->nrows; c0 += RAE_RK_ROWCHUNK) {
        const int n = (int)std::min<int64_t>(RAE_RK_ROWCHUNK, a->nrows - c0);
        e.row0 = a->row0 + c0;
        e.n = n;
        launch_enc_mt(e, st);
        RankArgs k = rank_queries_of(e, a, L.q, out->target ? out->target + 2 * c0 : nullptr, st);
        k.greater = out->greater + 2 * c0; k.equal = out->equal + 2 * c0;
        k.part = (float2*)(ws + L.o_part);
        float* lse = !want_lse ? nullptr : (out->lse ? out->lse + 2 * c0 : (float*)(ws + L.o_lse));
        rank_launch(k, lse, st);
        if (out->summary) {
            const int nblk = ceil_div(n, RAE_EV_SUMROWS);
            hipLaunchKernelGGL(k_rank_blocksum, dim3((unsigned)nblk), dim3(RAE_EV_BT), 0, st,
                               (const int32_t*)k.greater, (const int32_t*)k.equal,
                               (const float*)k.target, (const float*)lse, n, hk, partial);
            hipLaunchKernelGGL(k_rank_acc, dim3(1), dim3(64), 0, st, (const double*)partial, nblk,
                               out->summary, c0 == 0 ? 1 : 0);
        }
        HIPCHK(hipGetLastError());
    }
    return RAE_OK;
}

// ---- top-k entity retrieval ---------------------------------------------------------------------
namespace {
struct TopkLayout {                          // rae_eval_topk's workspace
    size_t o_keys, total;
    EncWs enc;
    QueryWs q;
};
// the strips' kept lists of one round of RAE_ETK_QCHUNK queries
inline size_t topk_keys_bytes(int64_t n, int top) {
    return ev_align((size_t)rank_strips(n) * RAE_ETK_QCHUNK * (size_t)top * sizeof(rae_key64));
}
int topk_top(int32_t top) {
    if (top < 1 || top > RAE_ETK_MAXTOP) return fail(RAE_E_INVALID, "top must be in [1, 32]");
    return RAE_OK;
}
// shapes of rae_eval_topk and its workspace layout (host only)
int eval_topk_layout(const rae_eval_args* a, int32_t top, TopkLayout& L) {
    if (const int rc = eval_shapes(a, false)) return rc;
    if (const int rc = entity_count(a->n_entities)) return rc;
    if (const int rc = topk_top(top)) return rc;
    const size_t ch = RAE_RK_ROWCHUNK;
    L.o_keys = lay_queries(a, ch, lay_enc(a, ch, 0, L.enc), L.q);
    L.total = L.o_keys + topk_keys_bytes(a->n_entities, top);
    return RAE_OK;
}
// k.nq queries on the stream in rounds of RAE_ETK_QCHUNK: selection per strip, then the merge
int topk_launch(RankArgs k, int64_t nq, int top, rae_key64* keys, int32_t* ents, float* scores,
                hipStream_t st) {
    const int strips = rank_strips(k.n);
    k.tps = rank_tiles_per_strip(k.n);
    k.ntiles = rank_tiles(k.n);
    k.target = nullptr; k.greater = nullptr; k.equal = nullptr; k.part = nullptr;
    const bool av4 = (k.r % 4) == 0;
    // large dynamic LDS is opted into per kernel (not a stream operation)
    HIPCHK(hipFuncSetAttribute(av4 ? (const void*)k_topk<true> : (const void*)k_topk<false>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, RAE_ETK_LDS_BYTES));
    const RankArgs base = k;
    for (int64_t c0 = 0; c0 < nq; c0 += RAE_ETK_QCHUNK) {
        k.Q = base.Q + c0 * base.ldq;
        k.add = base.add ? base.add + c0 : nullptr;
        k.skip = base.skip ? base.skip + c0 : nullptr;
        k.nq = (int)std::min<int64_t>(RAE_ETK_QCHUNK, nq - c0);
        TopkOut o;
        o.keys = keys; o.top = top;
        const dim3 grid((unsigned)ceil_div(k.nq, RAE_RK_TQ), (unsigned)strips);
        with_bool(av4, [&](auto V) {
            hipLaunchKernelGGL(k_topk<RAE_CV(V)>, grid, dim3(RAE_RK_BT), RAE_ETK_LDS_BYTES, st, k, o);
        });
        hipLaunchKernelGGL(k_topk_finish, dim3((unsigned)ceil_div(k.nq, RAE_ETK_FQ)),
                           dim3(RAE_ETK_FQ * 64), 0, st, (const rae_key64*)keys, strips, k.nq, top,
                           ents + c0 * top, scores ? scores + c0 * top : nullptr);
        HIPCHK(hipGetLastError());
    }
    return RAE_OK;
}
}  // namespace

extern "C" int64_t rae_topk_workspace_bytes(const rae_topk_args* q, const rae_eval_args* e,
                                            int32_t top) {
    if ((q != nullptr) == (e != nullptr))
        return fail(RAE_E_INVALID, "give exactly one of the two argument structs"), -1;
    if (q) {
        if (query_shapes(q->embed, q->n_entities) || topk_top(top)) return -1;
        return (int64_t)topk_keys_bytes(q->n_entities, top);
    }
    TopkLayout L;
    if (eval_topk_layout(e, top, L)) return -1;
    return (int64_t)L.total;
}

extern "C" int rae_topk_queries(const rae_topk_args* a, rae_stream_t stream) {
    if (!a) return fail(RAE_E_INVALID, "null argument");
    if (const int rc = query_shapes(a->embed, a->n_entities)) return rc;
    if (const int rc = topk_top(a->top)) return rc;
    if (a->nq < 0) return fail(RAE_E_INVALID, "nq must be >= 0");
    if (a->ldq < a->embed) return fail(RAE_E_INVALID, "ldq is smaller than embed");
    if (a->ldq % 4) return fail(RAE_E_INVALID, "ldq must be a multiple of 4");
    if (a->nq == 0) return RAE_OK;            // nothing is read or written
    if (!a->Q) return fail(RAE_E_INVALID, "Q is NULL");
    if ((uintptr_t)a->Q & 15) return fail(RAE_E_INVALID, "Q must be 16-byte aligned");
    if (!a->A) return fail(RAE_E_INVALID, "A is NULL");
    if ((a->embed % 4) == 0 && ((uintptr_t)a->A & 15))
        return fail(RAE_E_INVALID, "A must be 16-byte aligned");
    if (!a->ents_out) return fail(RAE_E_INVALID, "ents_out is NULL");
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes,
                                       topk_keys_bytes(a->n_entities, a->top),
                                       "rae_topk_workspace_bytes"))
        return rc;
    RankArgs k;
    k.Q = a->Q; k.ldq = a->ldq; k.add = a->add; k.skip = a->skip;
    k.A = a->A; k.Ab = a->Ab; k.n = a->n_entities; k.r = a->embed; k.nq = 0;
    return topk_launch(k, a->nq, a->top, (rae_key64*)a->workspace, a->ents_out, a->scores_out,
                       (hipStream_t)stream);
}

extern "C" int rae_eval_topk(const rae_eval_args* a, const rae_topk_out* out, rae_stream_t stream) {
    if (!out) return fail(RAE_E_INVALID, "out is NULL");
    TopkLayout L;
    if (const int rc = eval_topk_layout(a, out->top, L)) return rc;
    if (const int rc = check_rows(a)) return rc;
    if (const int rc = check_model(a)) return rc;
    if (a->nrows > 0 && !out->ents) return fail(RAE_E_INVALID, "ents is NULL");
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes, L.total,
                                       "rae_topk_workspace_bytes"))
        return rc;
    if (const int rc = check_align(a)) return rc;
    if (a->nrows == 0) return RAE_OK;         // nothing is written
    hipStream_t st = (hipStream_t)stream;
    const int top = out->top;
    if (const int rc = eval_large_lds((a->relations % 4) == 0 ? (const void*)k_rank_build<true>
                                                               : (const void*)k_rank_build<false>, a))
        return rc;
    EvalArgs e = eval_args_of(a, RAE_RK_ROWCHUNK, L.enc);   // the entropy term lands in terms, unread
    for (int64_t c0 = 0; c0 < a->nrows; c0 += RAE_RK_ROWCHUNK) {
        const int n = (int)std::min<int64_t>(RAE_RK_ROWCHUNK, a->nrows - c0);
        e.row0 = a->row0 + c0;
        e.n = n;
        launch_enc_mt(e, st);
        RankArgs k = rank_queries_of(e, a, L.q, nullptr, st);
        if (!out->skip_true) k.skip = nullptr;
        if (const int rc = topk_launch(k, 2 * (int64_t)n, top,
                                       (rae_key64*)((char*)a->workspace + L.o_keys),
                                       out->ents + 2 * c0 * top,
                                       out->scores ? out->scores + 2 * c0 * top : nullptr, st))
            return rc;
    }
    return RAE_OK;
}

// ---- relation scores from the decoder -----------------------------------------------------------
namespace {
struct RelLayout { size_t o_psi, o_lsm, total; };
int eval_rel_layout(const rae_eval_args* a, RelLayout& L) {
    if (const int rc = eval_shapes(a, false)) return rc;
    if (const int rc = entity_count(a->n_entities)) return rc;
    const size_t per = ev_align((size_t)RAE_RS_ROUND * a->relations * sizeof(float));
    L.o_psi = 0; L.o_lsm = per; L.total = 2 * per;
    return RAE_OK;
}
template <int NTA, int NTB, int TK>
int rel_launch_cfg(const RelArgs& k, dim3 grid, size_t lds, hipStream_t st) {
    if (lds > 48 * 1024)         // large dynamic LDS is opted into per kernel (not a stream operation)
        HIPCHK(hipFuncSetAttribute((const void*)k_relscore<NTA, NTB, TK>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_relscore<NTA, NTB, TK>), grid, dim3(RAE_RS_BT), lds, st, k);
    return RAE_OK;
}
// one round (k.nq <= RAE_RS_ROUND pairs) on the stream
int rel_launch(RelArgs k, hipStream_t st) {
    const int m = k.m, r = k.r;
    k.KR = k.dec == RAE_DEC_SP ? 0 : r * r;
    k.K = k.KR + (k.dec == RAE_DEC_RESCAL ? 0 : 2 * r);
    k.rinv = r > 1 ? (unsigned)((1ull << 32) / (unsigned)r) + 1u : 0u;
    k.av4 = (r % 4) == 0 && ((uintptr_t)k.A & 15) == 0;
    const RelConfig c = rel_config(m);
    const dim3 grid((unsigned)ceil_div(k.nq, rel_block_examples(c)),
                    (unsigned)ceil_div(m, rel_group_cols(c)));
    const size_t lds = rel_lds_bytes(c);
    switch (c.nta + c.ntb) {                 // the cases of rel_config
    case 1: return rel_launch_cfg<1, 0, 128>(k, grid, lds, st);
    case 2: return rel_launch_cfg<1, 1, 64>(k, grid, lds, st);
    case 4: return rel_launch_cfg<2, 2, 64>(k, grid, lds, st);
    case 7: return rel_launch_cfg<4, 3, 64>(k, grid, lds, st);
    case 8: return rel_launch_cfg<4, 4, 64>(k, grid, lds, st);
    case 12: return rel_launch_cfg<6, 6, 32>(k, grid, lds, st);
    case 16: return rel_launch_cfg<8, 8, 32>(k, grid, lds, st);
    default: return rel_launch_cfg<10, 10, 32>(k, grid, lds, st);
    }
}
}  // namespace

extern "C" int64_t rae_relscore_workspace_bytes(const rae_relscore_args* q, const rae_eval_args* e) {
    if ((q != nullptr) == (e != nullptr))
        return fail(RAE_E_INVALID, "give exactly one of the two argument structs"), -1;
    if (q) {
        if (rel_shapes(q->decoder, q->relations, q->embed, q->n_entities)) return -1;
        return 0;
    }
    RelLayout L;
    if (eval_rel_layout(e, L)) return -1;
    return (int64_t)L.total;
}

extern "C" int rae_relation_scores(const rae_relscore_args* a, rae_stream_t stream) {
    if (!a) return fail(RAE_E_INVALID, "null argument");
    if (const int rc = rel_shapes(a->decoder, a->relations, a->embed, a->n_entities)) return rc;
    if (a->nq < 0) return fail(RAE_E_INVALID, "nq must be >= 0");
    if (a->ldp < a->relations) return fail(RAE_E_INVALID, "ldp is smaller than relations");
    if (a->workspace_bytes < 0) return fail(RAE_E_INVALID, "workspace_bytes must be >= 0");
    if ((uintptr_t)a->workspace & 255) return fail(RAE_E_INVALID, "workspace must be 256-byte aligned");
    if (a->nq == 0) return RAE_OK;            // nothing is read or written
    const int m = a->relations, r = a->embed;
    const bool bil = a->decoder != RAE_DEC_SP;
    if (!a->A) return fail(RAE_E_INVALID, "A is NULL");
    if (a->decoder != RAE_DEC_RESCAL && (!a->C1 || !a->C2))
        return fail(RAE_E_INVALID, "C1 / C2 is NULL");
    if (bil && !a->R3) return fail(RAE_E_INVALID, "R3 is NULL");
    if (!a->e1 || !a->e2) return fail(RAE_E_INVALID, "e1 / e2 is NULL");
    if (!a->psi_out) return fail(RAE_E_INVALID, "psi_out is NULL");
    if ((m % 4) == 0 && (((uintptr_t)a->C1 | (uintptr_t)a->C2 | (uintptr_t)a->R3) & 15))
        return fail(RAE_E_INVALID, "C1 / C2 / R3 must be 16-byte aligned");
    if (((uintptr_t)a->A | (uintptr_t)a->psi_out | (uintptr_t)a->e1 | (uintptr_t)a->e2) & 3)
        return fail(RAE_E_INVALID, "A / psi_out / e1 / e2 must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (int64_t c0 = 0; c0 < a->nq; c0 += RAE_RS_ROUND) {
        RelArgs k;
        k.dec = a->decoder; k.m = m; k.r = r;
        k.A = a->A; k.C1 = a->C1; k.C2 = a->C2; k.R3 = a->R3;
        k.e1 = a->e1 + c0; k.e2 = a->e2 + c0; k.n_ent = a->n_entities;
        k.nq = (int)std::min<int64_t>(RAE_RS_ROUND, a->nq - c0);
        k.psi = a->psi_out + c0 * a->ldp; k.ldp = a->ldp;
        if (const int rc = rel_launch(k, st)) return rc;
        HIPCHK(hipGetLastError());
    }
    return RAE_OK;
}

extern "C" int rae_eval_relations(const rae_eval_args* a, const rae_rel_out* out, rae_stream_t stream) {
    RelLayout L;
    if (const int rc = eval_rel_layout(a, L)) return rc;
    if (!out) return fail(RAE_E_INVALID, "out is NULL");
    if (!out->psi && !out->joint && !out->labels_dec && !out->labels_joint)
        return fail(RAE_E_INVALID, "all four outputs are NULL");
    if (const int rc = check_rows(a)) return rc;
    if (const int rc = check_model(a)) return rc;
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes, L.total,
                                       "rae_relscore_workspace_bytes"))
        return rc;
    if (const int rc = check_align(a)) return rc;
    if (a->nrows == 0) return RAE_OK;         // nothing is read or written
    const int m = a->relations, r = a->embed;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)a->workspace;
    const bool want_joint = out->joint || out->labels_joint;
    const bool want_fin = want_joint || out->labels_dec;
    for (int64_t c0 = 0; c0 < a->nrows; c0 += RAE_RS_ROUND) {
        const int n = (int)std::min<int64_t>(RAE_RS_ROUND, a->nrows - c0);
        RelArgs k;
        k.dec = a->decoder; k.m = m; k.r = r;
        k.A = a->A; k.C1 = a->C1; k.C2 = a->C2; k.R3 = a->R3;
        k.e1 = a->args1 + a->row0 + c0; k.e2 = a->args2 + a->row0 + c0; k.n_ent = a->n_entities;
        k.nq = n;
        k.psi = out->psi ? out->psi + c0 * m : (float*)(ws + L.o_psi);
        k.ldp = m;
        if (const int rc = rel_launch(k, st)) return rc;
        const dim3 ge((unsigned)std::min(ceil_div(n, RAE_RS_EBT / RAE_WAVE), 65536));
        float* lsm = (float*)(ws + L.o_lsm);
        if (want_joint) {
            RelEnc e;
            e.indptr = a->indptr; e.indices = a->indices; e.values = a->values;
            e.W = a->W; e.Wb = a->Wb; e.m = m; e.row0 = a->row0 + c0; e.n = n; e.lsm = lsm;
            hipLaunchKernelGGL(k_rel_enc, ge, dim3(RAE_RS_EBT), 0, st, e);
        }
        if (want_fin) {
            RelFin f;
            f.psi = k.psi; f.ldp = m; f.lsm = want_joint ? lsm : nullptr; f.Ab = a->Ab;
            f.e1 = k.e1; f.e2 = k.e2; f.n_ent = a->n_entities; f.m = m; f.n = n;
            f.joint = out->joint ? out->joint + c0 * m : nullptr;
            f.labels_dec = out->labels_dec ? out->labels_dec + c0 : nullptr;
            f.labels_joint = out->labels_joint ? out->labels_joint + c0 : nullptr;
            hipLaunchKernelGGL(k_rel_fin, ge, dim3(RAE_RS_EBT), 0, st, f);
        }
        HIPCHK(hipGetLastError());
    }
    return RAE_OK;
}

// ---- cluster evaluation and profiles: what their entries share (host only) ---------------------
namespace {
// p[0, n) = 0 on the stream unless the entry accumulates; at most `cap` workgroups
template <class T> int zero_unless(bool accumulate, T* p, int64_t n, int64_t cap, hipStream_t st) {
    if (accumulate) return RAE_OK;
    const int64_t zg = std::min<int64_t>((n + 255) / 256, cap);
    hipLaunchKernelGGL(k_zero<T>, dim3((unsigned)zg), dim3(256), 0, st, p, (long long)n);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}
// row_pair_stream's head: the rows before the first index at which both pointers are 16-byte
// aligned (*gv); with none, the labels alone are aligned and `second` is read as dwords
int pair_head(const int64_t* labels, const int32_t* second, int64_t nrows, bool* gv) {
    int head = -1;
    for (int h = 0; h < 4; ++h)
        if ((((uintptr_t)(labels + h)) & 15) == 0 && (((uintptr_t)(second + h)) & 15) == 0) {
            head = h;
            break;
        }
    *gv = head >= 0;
    if (!*gv) head = ((uintptr_t)labels & 15) ? 1 : 0;
    return head > nrows ? (int)nrows : head;
}
}  // namespace

extern "C" int rae_cluster_count(const int64_t* labels, const int32_t* gold, int64_t nrows,
                                 int32_t relations, int32_t n_gold, int32_t form, int64_t* table,
                                 rae_stream_t stream) {
    if (const int rc = not_null({{labels, "labels"}, {gold, "gold"}, {table, "table"}})) return rc;
    if (const int rc = relations_range(relations)) return rc;
    if (n_gold < 0 || n_gold > 4095) return fail(RAE_E_INVALID, "n_gold must be in [0, 4095]");
    if (nrows < 0) return fail(RAE_E_INVALID, "nrows must be >= 0");
    const bool accumulate = (form & RAE_CCOUNT_ACCUMULATE) != 0;
    const int kind = form & ~RAE_CCOUNT_ACCUMULATE;
    if (kind != RAE_CCOUNT_AUTO && kind != RAE_CCOUNT_LDS && kind != RAE_CCOUNT_GLOBAL)
        return fail(RAE_E_INVALID, "form must be RAE_CCOUNT_AUTO, _LDS or _GLOBAL");
    const char* al = "labels / gold / table must be aligned to their element size";
    if (const int rc = aligned({labels, table}, 7, al)) return rc;
    if (const int rc = aligned({gold}, 3, al)) return rc;
    const int64_t cells = (int64_t)relations * (n_gold + 1);
    // a workgroup's 32-bit counters hold its share of the rows: nrows / 512 workgroups < 2^31
    const bool fits = cells <= RAE_CC_LDS_CELLS && nrows < (1ll << 40);
    if (kind == RAE_CCOUNT_LDS && !fits)
        return fail(RAE_E_INVALID, "form RAE_CCOUNT_LDS: relations * (n_gold + 1) counters exceed "
                                   "the LDS budget of 16384 (or nrows >= 2^40)");
    const bool lds = kind == RAE_CCOUNT_LDS || (kind == RAE_CCOUNT_AUTO && fits);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* tb = (unsigned long long*)table;
    if (const int rc = zero_unless(accumulate, tb, cells, 1024, st)) return rc;
    if (nrows == 0) return RAE_OK;
    bool gv;
    const int head = pair_head(labels, gold, nrows, &gv);
    const int64_t nq = (nrows - head) >> 2;
    const int64_t per = (int64_t)RAE_CC_BT * RAE_CC_QPT;
    int64_t grid = (nq + per - 1) / per;
    const int64_t cap = lds ? RAE_CC_GRID_LDS : RAE_CC_GRID_GLOBAL;
    grid = std::max<int64_t>(1, std::min(grid, cap));
    const size_t shmem = lds ? (size_t)cells * sizeof(unsigned) : 0;
    const void* fn = lds ? (gv ? (const void*)k_ccount<true, true> : (const void*)k_ccount<true, false>)
                         : (gv ? (const void*)k_ccount<false, true> : (const void*)k_ccount<false, false>);
    if (shmem > 48 * 1024)       // large dynamic LDS is opted into per kernel (not a stream operation)
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    with_bool(lds, [&](auto Lf) {
        with_bool(gv, [&](auto Gf) {
            hipLaunchKernelGGL((k_ccount<RAE_CV(Lf), RAE_CV(Gf)>), dim3((unsigned)grid),
                               dim3(RAE_CC_BT), shmem, st, (const long long*)labels,
                               (const int*)gold, (long long)nrows, head, (int)relations,
                               (int)n_gold, tb);
        });
    });
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

extern "C" int rae_b3_metrics(const int64_t* table, const int64_t* gold_sizes, int64_t n_assessable,
                              int32_t relations, int32_t n_gold, double* metrics_out,
                              int64_t* sizes_out, rae_stream_t stream) {
    if (const int rc = not_null({{table, "table"}, {metrics_out, "metrics_out"}})) return rc;
    if (const int rc = relations_range(relations)) return rc;
    if (n_gold < 0 || n_gold > 4095) return fail(RAE_E_INVALID, "n_gold must be in [0, 4095]");
    if (n_gold > 0 && !gold_sizes) return fail(RAE_E_INVALID, "gold_sizes is NULL");
    if (n_assessable < 0) return fail(RAE_E_INVALID, "n_assessable must be >= 0");
    if (const int rc = aligned({table, gold_sizes, metrics_out, sizes_out}, 7,
                               "table / gold_sizes / metrics_out / sizes_out must be 8-byte aligned"))
        return rc;
    hipLaunchKernelGGL(k_b3, dim3(1), dim3(RAE_B3_BT), 0, (hipStream_t)stream,
                       (const long long*)table, (const long long*)gold_sizes,
                       (long long)n_assessable, (int)relations, (int)n_gold, metrics_out,
                       (long long*)sizes_out);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

// ---- per-cluster trigger profiles -----------------------------------------------------------
extern "C" int rae_row_keys(const int32_t* indptr, const int32_t* indices, const float* values,
                            const int32_t* key_of_feature, int64_t n_features, int64_t row0,
                            int64_t nrows, int32_t* keys_out, rae_stream_t stream) {
    if (const int rc = not_null({{indptr, "indptr"}, {indices, "indices"},
                                 {key_of_feature, "key_of_feature"}, {keys_out, "keys_out"}}))
        return rc;
    if (const int rc = count_range("n_features", n_features, 0)) return rc;
    if (row0 < 0) return fail(RAE_E_INVALID, "row0 must be >= 0");
    if (const int rc = count_range("nrows", nrows, 0)) return rc;
    if (const int rc = aligned({indptr, indices, values, key_of_feature, keys_out}, 3,
                               "pointers must be 4-byte aligned"))
        return rc;
    if (nrows == 0) return RAE_OK;
    const int64_t per = 4 * (RAE_RWK_BT / 64);            // rows per workgroup and round
    const int64_t grid = std::min<int64_t>((nrows + per - 1) / per, 65536);
    hipLaunchKernelGGL(k_row_keys, dim3((unsigned)grid), dim3(RAE_RWK_BT), 0, (hipStream_t)stream,
                       indptr, indices, values, key_of_feature, (long long)n_features,
                       (long long)row0, (long long)nrows, keys_out);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

extern "C" int rae_cluster_key_count(const int64_t* labels, const int32_t* keys, int64_t nrows,
                                     int32_t relations, int32_t n_keys, int32_t accumulate,
                                     int32_t* counts, rae_stream_t stream) {
    if (const int rc = not_null({{labels, "labels"}, {keys, "keys"}, {counts, "counts"}})) return rc;
    if (const int rc = relations_range(relations)) return rc;
    if (const int rc = key_count(n_keys)) return rc;
    const int64_t cells = (int64_t)relations * n_keys;
    if (cells > (1ll << 27)) return fail(RAE_E_INVALID, "relations * n_keys must be <= 2^27");
    if (const int rc = count_range("nrows", nrows, 0)) return rc;
    const char* al = "labels / keys / counts must be aligned to their element size";
    if (const int rc = aligned({labels}, 7, al)) return rc;
    if (const int rc = aligned({keys, counts}, 3, al)) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned* ct = (unsigned*)counts;
    if (const int rc = zero_unless(accumulate != 0, ct, cells, 4096, st)) return rc;
    if (nrows == 0) return RAE_OK;
    bool gv;
    const int head = pair_head(labels, keys, nrows, &gv);
    const int64_t nq = (nrows - head) >> 2;
    const int64_t per = (int64_t)RAE_CK_BT * RAE_CK_QPT;
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((nq + per - 1) / per, RAE_CK_GRID));
    with_bool(gv, [&](auto Gf) {
        hipLaunchKernelGGL((k_ckcount<RAE_CV(Gf)>), dim3((unsigned)grid), dim3(RAE_CK_BT), 0, st,
                           (const long long*)labels, (const int*)keys, (long long)nrows, head,
                           (int)relations, (int)n_keys, ct);
    });
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

extern "C" int rae_cluster_topk(const int32_t* counts, int32_t relations, int32_t n_keys,
                                int64_t ld, int32_t top, int32_t* keys_out, int32_t* counts_out,
                                rae_stream_t stream) {
    if (const int rc = not_null({{counts, "counts"}, {keys_out, "keys_out"},
                                 {counts_out, "counts_out"}}))
        return rc;
    if (const int rc = relations_range(relations)) return rc;
    if (const int rc = key_count(n_keys)) return rc;
    if (ld < n_keys) return fail(RAE_E_INVALID, "ld must be >= n_keys");
    if (top < 1 || top > RAE_TK_MAXTOP) return fail(RAE_E_INVALID, "top must be in [1, 32]");
    if (const int rc = aligned({counts, keys_out, counts_out}, 3,
                               "counts / keys_out / counts_out must be 4-byte aligned"))
        return rc;
    hipLaunchKernelGGL(k_ctopk, dim3((unsigned)relations), dim3(RAE_TK_BT), 0, (hipStream_t)stream,
                       (const int*)counts, (int)n_keys, (long long)ld, (int)top, keys_out,
                       counts_out);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

// ---- relation feature profiles (rae_feature.hpp) ----------------------------------------------
extern "C" int rae_feature_support(const int32_t* indptr, const int32_t* indices,
                                   const float* values, int64_t n_features, int64_t row0,
                                   int64_t nrows, int32_t accumulate, int32_t* support,
                                   rae_stream_t stream) {
    if (const int rc = not_null({{indptr, "indptr"}, {indices, "indices"}, {support, "support"}}))
        return rc;
    if (const int rc = count_range("n_features", n_features, 0)) return rc;
    if (row0 < 0) return fail(RAE_E_INVALID, "row0 must be >= 0");
    if (const int rc = count_range("nrows", nrows, 0)) return rc;
    if (const int rc = aligned({indptr, indices, values, support}, 3,
                               "indptr / indices / values / support must be 4-byte aligned"))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned* sp = (unsigned*)support;
    if (n_features == 0) return RAE_OK;       // no cell to zero or count
    if (const int rc = zero_unless(accumulate != 0, sp, n_features, 4096, st)) return rc;
    if (nrows == 0) return RAE_OK;
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(ceil_div(nrows, (int64_t)RAE_FS_ROWS),
                                                                RAE_FS_GRID));
    // values by 16-byte loads when they are aligned where the indices are
    const int vm = !values ? 0 : ((((uintptr_t)values ^ (uintptr_t)indices) & 15) == 0 ? 1 : 2);
    with_vm(vm, [&](auto Vm) {
        hipLaunchKernelGGL(k_fsupport<RAE_CV(Vm)>, dim3((unsigned)grid), dim3(RAE_FS_BT), 0, st,
                           indptr, indices, values, (long long)n_features, (long long)row0,
                           (long long)nrows, sp);
    });
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

namespace {
struct FtopkLayout { size_t o_keys, o_mean, total; int strips; };
// shapes of rae_feature_topk and its workspace layout (host only)
int ftopk_layout(const rae_ftopk_args* a, FtopkLayout& L) {
    if (!a) return fail(RAE_E_INVALID, "null argument");
    if (const int rc = relations_range(a->relations)) return rc;
    if (const int rc = count_range("n_features", a->n_features, 0)) return rc;
    if (a->ldw < a->relations) return fail(RAE_E_INVALID, "ldw is smaller than relations");
    if (const int rc = topk_top(a->top)) return rc;
    if (a->centre != 0 && a->centre != 1) return fail(RAE_E_INVALID, "centre must be 0 or 1");
    L.strips = ftopk_strips(a->n_features);
    L.o_keys = 0;
    L.o_mean = ev_align((size_t)L.strips * (size_t)a->relations * (size_t)a->top * sizeof(rae_key64));
    L.total = L.o_mean + (a->centre ? ev_align((size_t)a->n_features * sizeof(double)) : 0);
    return RAE_OK;
}
}  // namespace

extern "C" int64_t rae_feature_topk_workspace_bytes(const rae_ftopk_args* a) {
    FtopkLayout L;
    if (ftopk_layout(a, L)) return -1;
    return (int64_t)L.total;
}

extern "C" int rae_feature_topk(const rae_ftopk_args* a, rae_stream_t stream) {
    FtopkLayout L;
    if (const int rc = ftopk_layout(a, L)) return rc;
    if (a->n_features > 0 && !a->W) return fail(RAE_E_INVALID, "W is NULL");
    if (!a->feats_out) return fail(RAE_E_INVALID, "feats_out is NULL");
    if (const int rc = aligned({a->W, a->support, a->feats_out, a->scores_out}, 3,
                               "W / support / feats_out / scores_out must be 4-byte aligned"))
        return rc;
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes, L.total,
                                       "rae_feature_topk_workspace_bytes"))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)a->workspace;
    FtopkArgs k;
    k.W = a->W; k.d = a->n_features; k.ldw = a->ldw; k.strip_rows = ftopk_strip_rows(a->n_features);
    k.m = a->relations; k.top = a->top; k.min_support = a->min_support;
    k.support = a->centre ? nullptr : a->support;
    k.mean = a->centre ? (const double*)(ws + L.o_mean) : nullptr;
    k.keys = (rae_key64*)(ws + L.o_keys);
    if (a->centre && a->n_features > 0) {
        const int64_t per = (int64_t)(RAE_FR_BT / 64) * RAE_FR_ROWS;
        const int64_t gr = std::min<int64_t>(ceil_div(a->n_features, per), RAE_FR_GRID);
        hipLaunchKernelGGL(k_frowstat, dim3((unsigned)gr), dim3(RAE_FR_BT), 0, st, a->W,
                           (long long)a->n_features, (int)a->relations, (long long)a->ldw,
                           a->support, (int)a->min_support, (double*)(ws + L.o_mean));
    }
    const dim3 grid((unsigned)ceil_div((int)a->relations, 64), (unsigned)L.strips);
    with_bool(a->centre != 0, [&](auto Cf) {
        hipLaunchKernelGGL(k_ftopk<RAE_CV(Cf)>, grid, dim3(RAE_FT_BT), 0, st, k);
    });
    hipLaunchKernelGGL(k_ftopk_finish, dim3((unsigned)ceil_div((int)a->relations, RAE_FT_FQ)),
                       dim3(RAE_FT_FQ * 64), 0, st, (const rae_key64*)k.keys, L.strips,
                       (int)a->relations, (int)a->top, a->feats_out, a->scores_out);
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

// ---- cluster exemplars (rae_exemplar.hpp) -------------------------------------------------------
extern "C" int rae_label_stats(const int32_t* indptr, const int32_t* indices, const float* values,
                               const float* W, const float* Wb, int32_t relations, int64_t row0,
                               int64_t nrows, int64_t* labels_out, float* margin_out,
                               float* pmax_out, rae_stream_t stream) {
    if (const int rc = not_null({{indptr, "indptr"}, {indices, "indices"}, {W, "W"}, {Wb, "Wb"},
                                 {labels_out, "labels_out"}}))
        return rc;
    const int m = relations;
    if (m < 1 || m > 512) return fail(RAE_E_INVALID, "relations must be in [1, 512] for labelling");
    const bool v4 = (m % 4) == 0;
    if (!v4 && m > 128)
        return fail(RAE_E_INVALID, "relations must be a multiple of 4 above 128 for labelling");
    if (row0 < 0) return fail(RAE_E_INVALID, "row0 must be >= 0");
    if (const int rc = count_range("nrows", nrows, 0)) return rc;
    if (v4)
        if (const int rc = aligned({W, Wb}, 15, "W / Wb must be 16-byte aligned")) return rc;
    if (const int rc = aligned({indptr, indices, values, W, Wb, margin_out, pmax_out}, 3,
                               "indptr / indices / values / W / Wb / margin_out / pmax_out must be "
                               "4-byte aligned"))
        return rc;
    if (const int rc = aligned({labels_out}, 7, "labels_out must be 8-byte aligned")) return rc;
    if (nrows == 0) return RAE_OK;
    const int64_t blocks = std::min<int64_t>((nrows + RAE_NWAVE - 1) / RAE_NWAVE, 65536);
    with_bool(v4, [&](auto Vf) {
        hipLaunchKernelGGL(k_label_stats<RAE_CV(Vf)>, dim3((unsigned)blocks), dim3(RAE_BT), 0,
                           (hipStream_t)stream, indptr, indices, values, W, Wb, m, row0, nrows,
                           labels_out, margin_out, pmax_out);
    });
    HIPCHK(hipGetLastError());
    return RAE_OK;
}

namespace {
struct CexLayout { size_t total; int strips, waves; };
// shapes of rae_cluster_exemplars and its workspace layout (host only)
int cex_layout(const rae_exemplar_args* a, CexLayout& L) {
    if (!a) return fail(RAE_E_INVALID, "null argument");
    if (const int rc = count_range("nrows", a->nrows, 0)) return rc;
    if (const int rc = relations_range(a->relations)) return rc;
    if (a->top < 1 || a->top > RAE_CX_MAXTOP) return fail(RAE_E_INVALID, "top must be in [1, 32]");
    if (a->largest != 0 && a->largest != 1) return fail(RAE_E_INVALID, "largest must be 0 or 1");
    L.strips = cex_strips(a->nrows);
    L.waves = cex_waves(a->relations, a->top);
    L.total = ev_align((size_t)L.strips * (size_t)a->relations * (size_t)a->top * sizeof(rae_key64));
    return RAE_OK;
}
}  // namespace

extern "C" int64_t rae_cluster_exemplars_workspace_bytes(const rae_exemplar_args* a) {
    CexLayout L;
    if (cex_layout(a, L)) return -1;
    return (int64_t)L.total;
}

extern "C" int rae_cluster_exemplars(const rae_exemplar_args* a, rae_stream_t stream) {
    CexLayout L;
    if (const int rc = cex_layout(a, L)) return rc;
    if (a->nrows > 0)
        if (const int rc = not_null({{a->labels, "labels"}, {a->scores, "scores"}})) return rc;
    if (!a->rows_out) return fail(RAE_E_INVALID, "rows_out is NULL");
    const char* al = "labels / scores / rows_out / scores_out must be aligned to their element size";
    if (const int rc = aligned({a->labels}, 7, al)) return rc;
    if (const int rc = aligned({a->scores, a->rows_out, a->scores_out}, 3, al)) return rc;
    if (const int rc = check_workspace(a->workspace, a->workspace_bytes, L.total,
                                       "rae_cluster_exemplars_workspace_bytes"))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    CexArgs k;
    k.labels = (const long long*)a->labels;
    k.scores = (const int*)a->scores;             // the scores' dwords, a bit cast
    k.nrows = a->nrows; k.strip_rows = cex_strip_rows(a->nrows);
    k.m = a->relations; k.top = a->top; k.negate = a->largest ? 0 : 1;
    k.keys = (rae_key64*)a->workspace;
    const size_t shmem = (size_t)L.waves * a->relations * a->top * sizeof(rae_key64);
    if (shmem > 48 * 1024)       // large dynamic LDS is opted into per kernel (not a stream operation)
        HIPCHK(hipFuncSetAttribute((const void*)k_cexemplar,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(k_cexemplar, dim3((unsigned)L.strips), dim3(L.waves * 64), shmem, st, k);
    hipLaunchKernelGGL(k_ftopk_finish, dim3((unsigned)ceil_div((int)a->relations, RAE_FT_FQ)),
                       dim3(RAE_FT_FQ * 64), 0, st, (const rae_key64*)k.keys, L.strips,
                       (int)a->relations, (int)a->top, a->rows_out, a->scores_out);
    if (k.negate && a->scores_out) {
        const int n = a->relations * a->top;
        hipLaunchKernelGGL(k_cex_negate, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st,
                           (const int32_t*)a->rows_out, a->scores_out, n);
    }
    HIPCHK(hipGetLastError());
    return RAE_OK;
}
