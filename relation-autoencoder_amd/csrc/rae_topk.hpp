// rae_topk_queries / rae_eval_topk: the `top` best-scoring entities of every query with their
// scores (argument prediction, selectional preferences of an induced relation).  The scores are
// rae_rank.hpp's: the same tile, slab loads and strip decomposition, a copy of its K loop
// (topk_tile_acc below says why a copy) and the same epilogue expression
// acc + (c + Ab[e]), so a score has the bits rae_rank_queries compares.  The (nq x n) matrix is
// never stored: a selection epilogue keeps the best `top` of every query in LDS.
//
// A candidate is the packed 64-bit key  orderable(score) << 32 | ~entity  (rae_key.hpp topk_key):
// unsigned 64-bit order is score descending, then entity ascending -- a total order.  A NaN score
// is no candidate, and 0 means "no entry".
//
// Kernels:
//   k_topk         workgroup (query tile, strip) as k_rank.  Per query of the workgroup LDS holds
//                  a kept list of `top` keys, sorted descending and zero-filled, a pending buffer
//                  of 64 keys with a counter, and the admission threshold = kept[top - 1] (0 until
//                  the list is full).  The epilogue runs in two phases per tile, one per 32-entity
//                  sub-tile of the entity waves: a lane packs its 16 scores of a query and appends
//                  the keys above the query's threshold to its pending buffer through the LDS
//                  counter (a query meets 2 waves x 2 lane halves x 16 = 64 candidates a phase:
//                  the buffer cannot overflow).  After a barrier wave w compacts queries
//                  [32 w, 32 w + 32), one query at a time across its lanes and only those with
//                  something pending (ballot): lane j holds kept[j] and pending[j]; the pending
//                  keys are read lane by lane (v_readlane, no LDS latency in the loop) and every
//                  key counts the larger ones, a pending key's rank among the kept ones being a
//                  ballot's popcount; the keys of rank < top are written to kept[rank], the
//                  threshold is refreshed and the counter cleared.  At the end of the strip the
//                  wave writes its queries' kept lists to keys[strip][query][top].
//                  LDS: slabs and Ab 33.5 KiB, kept 128 x 33 x 8 B = 33 KiB, pending
//                  128 x 65 x 8 B = 65 KiB (odd row strides in 8-byte words: the 32 queries of a
//                  wave instruction land in 32 bank pairs), thresholds 1 KiB, counters 0.5 KiB:
//                  133 KiB of gfx950's 160 KiB.  The 64 accumulators already hold the kernel at
//                  one workgroup per CU, so the LDS costs no residency.
//   k_topk_finish  one wave per query: the strips' lists are merged in strip order (two sorted
//                  lists of distinct keys in the two lane halves: rank = own index + the count of
//                  larger keys in the other half, read lane by lane; the next strip's list is
//                  loaded under the merge), the keys un-packed to (entity, score bits), padding
//                  (-1, -inf).
// Determinism: the order in which lanes append to a pending buffer is not fixed, but a phase's
// result is the set of the `top` largest keys of kept + pending, written in sorted order; keys
// are distinct (distinct entities) and totally ordered, so that set and its order are unique
// whatever the append order.  The kept list after a strip is therefore the strip's `top` largest
// keys, and the merged list the `top` largest of all: a function of the query's scores alone.
// A score is a function of its Q row, its A row, r, add and Ab (rae_rank.hpp), so an output row
// does not depend on nq, the query's slot or the other queries.
#pragma once
#include "rae_key.hpp"
#include "rae_rank.hpp"

namespace rae {

#define RAE_ETK_MAXTOP 32         // largest `top`
#define RAE_ETK_PEND 64           // pending keys per query and phase
#define RAE_ETK_LDKEPT 33         // row stride of the kept lists, keys
#define RAE_ETK_LDPEND 65         // row stride of the pending buffers, keys
#define RAE_ETK_QCHUNK 1024       // queries per launch round (the workspace's query extent)
#define RAE_ETK_FQ 4              // queries (waves) per k_topk_finish workgroup
#define RAE_ETK_LDS_BYTES                                                                       \
    ((RAE_RK_TQ * (RAE_ETK_LDKEPT + RAE_ETK_LDPEND + 1)) * 8 +                                  \
     (RAE_RK_TQ * RAE_RK_LDK + RAE_RK_TE * RAE_RK_LDK + RAE_RK_TE) * 4 + RAE_RK_TQ * 4)

struct TopkOut {
    rae_key64* keys;              // (strips, RAE_ETK_QCHUNK, top)
    int top;
};

// acc[entity tile][query tile] = the products <Q[q], A[e]> of the 128 x 128 tile at (q0, e0).
// This is rank_scores' K loop, statement for statement (rank_load / rank_store shared): factoring
// the loop out of rank_scores into one function moved k_rank's register allocation (207 -> 223
// VGPRs without the log-sum-exp), so k_rank keeps its loop and this is the copy.  The two must
// stay identical: tests/test_gpu_topk.py asks rae_rank_queries to find every returned score.
// The first barrier inside covers the caller's reads of the previous tile's slabs and sAb.
template <bool AV4>
__device__ __forceinline__ void topk_tile_acc(const RankArgs& a, float* sQ, float* sA, float* sAb,
                                              int q0, int64_t e0, const float* bq0,
                                              const float* bq1, const float* ba0,
                                              const float* ba1, rae_rk16 (&acc)[2][2]) {
    const int tid = threadIdx.x;
    const int r = a.r;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
    float4 pq[4], pa[4];
    rank_load<AV4>(a, q0, e0, 0, pq, pa);
    for (int k0 = 0; k0 < r; k0 += RAE_RK_TK) {
        __syncthreads();                      // the previous slab (and epilogue) is read
        rank_store(sQ, sA, pq, pa);
        if (k0 == 0 && tid < RAE_RK_TE)
            sAb[tid] = (a.Ab && e0 + tid < a.n) ? a.Ab[e0 + tid] : 0.f;
        __syncthreads();
        if (k0 + RAE_RK_TK < r) rank_load<AV4>(a, q0, e0, k0 + RAE_RK_TK, pq, pa);
        const int nk8 = (min(RAE_RK_TK, r - k0) + 7) >> 3;
        for (int k8 = 0; k8 < nk8; ++k8) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int kc = 8 * k8 + 2 * kk;
                const float b0 = bq0[kc], b1 = bq1[kc];
                const float a0 = ba0[kc], a1 = ba1[kc];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
}

// wave w: the queries [32 w, 32 w + 32) that have pending keys, one at a time across the lanes
__device__ __forceinline__ void topk_compact(rae_key64* sKept, rae_key64* sPend, rae_key64* sThr,
                                             int* sCnt, int w, int lane, int top) {
    const int mine = sCnt[w * 32 + (lane & 31)];
    unsigned todo = (unsigned)__ballot(mine > 0);             // lanes 0..31: one bit per query
    while (todo) {
        const int j = __builtin_ctz(todo);
        todo &= todo - 1;
        const int q = w * 32 + j;
        const int cnt = min(__builtin_amdgcn_readlane(mine, j), RAE_ETK_PEND);
        rae_key64* kept = sKept + q * RAE_ETK_LDKEPT;
        const rae_key64* pend = sPend + q * RAE_ETK_LDPEND;
        const rae_key64 ka = lane < top ? kept[lane] : 0ull;  // lanes >= top and empty slots: 0
        const rae_key64 kb = lane < cnt ? pend[lane] : 0ull;
        // pending key i is read from its lane (no LDS latency in the loop): the kept and the
        // pending keys count it if it is larger; its own rank among the kept keys is a ballot
        int ra = lane, rb = 0, rbk = 0;                       // kept is sorted: lane = rank in it
        for (int i = 0; i < cnt; ++i) {
            const rae_key64 p = topk_lane_key(kb, i);
            ra += p > ka ? 1 : 0;
            rb += p > kb ? 1 : 0;
            const int above = __popcll(__ballot(ka > p));
            rbk = lane == i ? above : rbk;
        }
        rb += rbk;
        __builtin_amdgcn_wave_barrier();                      // every lane has read: now rewrite
        if (ka != 0ull && ra < top) {
            kept[ra] = ka;
            if (ra == top - 1) sThr[q] = ka;
        }
        if (kb != 0ull && rb < top) {
            kept[rb] = kb;
            if (rb == top - 1) sThr[q] = kb;
        }
        if (lane == 0) sCnt[q] = 0;
        __builtin_amdgcn_wave_barrier();
    }
}

// AV4 as in rank_scores; smem: RAE_ETK_LDS_BYTES
template <bool AV4>
__device__ __forceinline__ void topk_scores(const RankArgs& a, const TopkOut& o, char* smem) {
    // the slabs first, at k_rank's offsets: below 64 KiB the K loop's operand reads can take
    // their offsets as immediates (ds_read2_b32, as in k_rank)
    float* sQ = reinterpret_cast<float*>(smem);
    float* sA = sQ + RAE_RK_TQ * RAE_RK_LDK;
    float* sAb = sA + RAE_RK_TE * RAE_RK_LDK;
    int* sCnt = reinterpret_cast<int*>(sAb + RAE_RK_TE);
    rae_key64* sKept = reinterpret_cast<rae_key64*>(sCnt + RAE_RK_TQ);     // byte 34816
    rae_key64* sPend = sKept + RAE_RK_TQ * RAE_ETK_LDKEPT;
    rae_key64* sThr = sPend + RAE_RK_TQ * RAE_ETK_LDPEND;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = w >> 1, we = w & 1;
    const int l31 = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * RAE_RK_TQ;
    const int strip = blockIdx.y;
    const int t0 = strip * a.tps, t1 = min(t0 + a.tps, a.ntiles);
    const unsigned nU = (unsigned)a.n;
    const int top = o.top;
    for (int i = tid; i < RAE_RK_TQ * RAE_ETK_LDKEPT; i += RAE_RK_BT) sKept[i] = 0ull;
    if (tid < RAE_RK_TQ) {
        sThr[tid] = 0ull;
        sCnt[tid] = 0;
    }                                             // ordered by the first tile's barriers
    float c[2];
    unsigned sk[2];
    int ql[2];
    bool qv[2];
#pragma unroll
    for (int tq = 0; tq < 2; ++tq) {
        ql[tq] = wq * 64 + tq * 32 + l31;
        const int q = q0 + ql[tq];
        const int qq = q < a.nq ? q : 0;
        qv[tq] = q < a.nq;
        c[tq] = a.add ? a.add[qq] : 0.f;
        sk[tq] = a.skip ? (unsigned)a.skip[qq] : 0xffffffffu;
    }
    const float* bq0 = sQ + (wq * 64 + l31) * RAE_RK_LDK + h;
    const float* bq1 = bq0 + 32 * RAE_RK_LDK;
    const float* ba0 = sA + (we * 64 + l31) * RAE_RK_LDK + h;
    const float* ba1 = ba0 + 32 * RAE_RK_LDK;
    for (int t = t0; t < t1; ++t) {
        const int64_t e0 = (int64_t)t * RAE_RK_TE;
        rae_rk16 acc[2][2];                       // [entity tile][query tile]
        topk_tile_acc<AV4>(a, sQ, sA, sAb, q0, e0, bq0, bq1, ba0, ba1, acc);
        // ---- selection: lane (l31, h) holds, of query tile tq, the scores of entities
        // e0 + 64 we + 32 te + (reg & 3) + 8 (reg >> 2) + 4 h; one phase per te
#pragma unroll
        for (int te = 0; te < 2; ++te) {
#pragma unroll
            for (int tq = 0; tq < 2; ++tq) {
                const rae_key64 thr = sThr[ql[tq]];
                rae_key64* pend = sPend + ql[tq] * RAE_ETK_LDPEND;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int eo = we * 64 + te * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const unsigned e = (unsigned)e0 + (unsigned)eo;
                    const float g = acc[te][tq][reg] + (c[tq] + sAb[eo]);
                    const bool ok = qv[tq] && e < nU && e != sk[tq] && g == g;
                    const rae_key64 key = topk_key(g, e);
                    if (ok && key > thr) {
                        const int pos = atomicAdd(sCnt + ql[tq], 1);
                        if (pos < RAE_ETK_PEND) pend[pos] = key;
                    }
                }
            }
            __syncthreads();                      // the phase's pending keys are in LDS
            topk_compact(sKept, sPend, sThr, sCnt, w, lane, top);
            // te == 0: the thresholds of the next phase; te == 1: the next tile's barriers, and
            // a wave writes out only the queries it compacts itself
            if (te == 0) __syncthreads();
        }
    }
    // ---- the strip's lists of this wave's 32 queries
    for (int j = 0; j < 32; ++j) {
        const int ql2 = w * 32 + j;
        const int q = q0 + ql2;
        if (q < a.nq && lane < top)
            o.keys[((int64_t)strip * RAE_ETK_QCHUNK + q) * top + lane] =
                sKept[ql2 * RAE_ETK_LDKEPT + lane];
    }
}

// one wave per query: sList holds 32 keys per wave (the merged list while it is rewritten)
__device__ __forceinline__ void topk_finish(const rae_key64* __restrict__ keys, int strips, int nq,
                                            int top, int32_t* __restrict__ ents,
                                            float* __restrict__ scores, rae_key64* sList) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = blockIdx.x * RAE_ETK_FQ + w;
    if (q >= nq) return;                          // the whole wave; no workgroup barrier below
    rae_key64* L = sList + w * 32;
    const int l31 = lane & 31;
    const bool lo = lane < 32;
    const rae_key64* mine = keys + (int64_t)q * top + l31;
    const int64_t step = (int64_t)RAE_ETK_QCHUNK * top;
    // both lane halves hold the merged list (sorted, zero-filled); the upper half takes the
    // strip's list for the merge, and the next strip's is loaded under it
    rae_key64 cur = l31 < top ? mine[0] : 0ull;
    rae_key64 nxt = (l31 < top && strips > 1) ? mine[step] : 0ull;
    for (int s = 1; s < strips; ++s) {
        const rae_key64 x = lo ? cur : nxt;
        if (s + 1 < strips && l31 < top) nxt = mine[(int64_t)(s + 1) * step];
        int rk = l31;                             // both lists are sorted: the rank in its own
        for (int i = 0; i < top; ++i) {           // ... plus the larger keys of the other list
            const rae_key64 pa = topk_lane_key(x, i), pb = topk_lane_key(x, 32 + i);
            rk += (lo ? pb : pa) > x ? 1 : 0;
        }
        if (lo) L[lane] = x;                      // slots the merge does not fill keep the old list
        __builtin_amdgcn_wave_barrier();
        if (x != 0ull && rk < top) L[rk] = x;
        __builtin_amdgcn_wave_barrier();
        cur = L[l31];
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < top) key_unpack_store(cur, ents, scores, (long long)q * top + lane);
}

}  // namespace rae
