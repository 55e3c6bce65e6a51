// rae_eval_cost: the forward-only objective over any row range of any split (no reference
// counterpart: the reference's Theano function fuses the update, learning/OieInduction.py:146-149).
// Per example b the three terms of the reference's all_scores grouped by example
// (learning/OieModel.py:80-90, the decoders' get_scores):
//   pos_b = logsig(u_b) + logsig(u_{l+b}),  H_b = alpha (-sum_k P log P),  neg_b = sum of the
//   example's 2s values logsig(-g)
// with the training kernels' stable forms (log-softmax, -softplus).  No exchange record, no
// backward, no parameter or accumulator write.
//
// Kernels (a chunk of examples per launch; the host loop walks the row range):
//   k_eval_dec   one workgroup per tile of RAE_EV_TE = 16 examples.
//                SP: the encoder (k_label's gather: one wave per example, several W-row loads
//                in flight) leaves the tile's P in LDS; wC1 / wC2 = P.C^T for the whole tile
//                on v_mfma_f32_16x16x4_f32 (C1 / C2 read once per tile); then per example the
//                1 + 2s A-row gathers, four rows per wave instruction (16 lanes per row, float4
//                columns when r % 4 == 0), dots against the tile's LDS vectors, log-sigmoids.
//                RESCAL / hybrid: the tile's v = M a2 and w = M^T a1 are the sums, in block
//                order, of k_eval_mt's partials (hybrid: + wC1 / wC2), then the same gathers.
//   k_eval_enc   RESCAL / hybrid: encoder of the chunk, P to the workspace, H to the terms.
//   k_eval_mt    RESCAL / hybrid: k_bil_mt's fp32 block scheme without its backward: workgroup
//                (it, jt) stages R[i0..i0+7][j0..j0+15][0..m) in LDS once per chunk, every wave
//                takes 16-example tiles, D[j][b] = sum_k R[i][j][k] P_bk per i, contracted at
//                once with a2 (over j) and a1 (over i); M never materialised, R read once per
//                chunk of RAE_EV_CHUNK_BIL examples.
//   k_eval_blocksum / k_eval_acc   the three column sums in double: one partial per 1024 rows
//                (a fixed in-block tree), the partials added in row order -- a function of the
//                term values and nrows only.
// Determinism: an example's arithmetic never depends on its slot in a tile (one wave / one
// 16-lane group / one MFMA column per example, the same instruction sequence in every slot),
// partial sums are combined in block order.
#pragma once
#include "rae_common.hpp"
#include "rae_label.hpp"

namespace rae {

#define RAE_EV_TE 16              // examples per k_eval_dec tile (one MFMA tile of columns)
#define RAE_EV_BT 256             // threads per k_eval_dec / k_eval_enc workgroup
#define RAE_EV_NW (RAE_EV_BT / RAE_WAVE)
#define RAE_EV_MTI 8              // k_eval_mt block: rows i
#define RAE_EV_MTJ 16             //                  columns j
#define RAE_EV_MTT 512            // threads per k_eval_mt workgroup
#define RAE_EV_MTW (RAE_EV_MTT / RAE_WAVE)
#define RAE_EV_SUMROWS 1024       // rows per partial of the column sums
#define RAE_EV_CHUNK_SP 65536     // examples per launch round, SP (a multiple of RAE_EV_SUMROWS)
#define RAE_EV_CHUNK_BIL 2048     // ... RESCAL / hybrid (bounds the partials in the workspace)

typedef float rae_ev4 __attribute__((ext_vector_type(4)));

struct EvalArgs {
    int dec, m, r, s;
    float alpha;
    const float *W, *Wb, *A, *Ab, *C1, *C2, *R3;
    const int32_t *indptr, *indices;
    const float* values;
    const int32_t *args1, *args2, *neg1, *neg2;
    int64_t neg_stride;
    int64_t row0;                 // split row of the chunk's first example
    int n;                        // examples of the chunk
    int cap;                      // example stride of the partials (the chunk capacity)
    int r4;                       // r rounded up to 4: row stride of the partials
    float* terms;                 // (n, 3) of the chunk
    float* P;                     // (n, m) of the chunk (RESCAL / hybrid)
    float* vpart;                 // (nbj, cap, r4): partials of M a2 per j-block
    float* wpart;                 // (nbi, cap, r4): partials of M^T a1 per i-block
};

__host__ __device__ inline int eval_r4(int r) { return (r + 3) & ~3; }
__host__ __device__ inline int eval_nbi(int r) { return (r + RAE_EV_MTI - 1) / RAE_EV_MTI; }
__host__ __device__ inline int eval_nbj(int r) { return (r + RAE_EV_MTJ - 1) / RAE_EV_MTJ; }
// floats of LDS of one k_eval_dec tile: P, the two contraction vectors per example, the
// hybrid's wC1 / wC2
__host__ __device__ inline size_t eval_dec_lds_floats(int dec, int m, int r) {
    const size_t mS = (size_t)((m + 3) & ~3), r4 = (size_t)eval_r4(r);
    return RAE_EV_TE * (mS + (dec == 2 ? 4 : 2) * r4);
}
__host__ __device__ inline size_t eval_mt_lds_bytes(int m) {
    return (size_t)RAE_EV_MTI * RAE_EV_MTJ * m * 4;
}

// log(sigmoid(x)) = -softplus(-x)
__device__ __forceinline__ float eval_logsig(float x) {
    float sig, sp;
    sigmoid_softplus(-x, sig, sp);
    return -sp;
}

// Encoder of one example by one wave (k_label's gather): P (m floats) to Pout (LDS or global,
// 16-byte aligned when V4); returns alpha H, identical in every lane.
template <bool V4>
__device__ __forceinline__ float eval_encode(const EvalArgs& a, int64_t ex, float* Pout) {
    typedef typename VecT<V4>::T VT;
    constexpr int VW = V4 ? 4 : 1;
    constexpr int U = 4;                         // load rounds in flight
    const int lane = threadIdx.x & 63;
    const int m = a.m, mv = m / VW;
    const int LPR = mv <= 16 ? 16 : (mv <= 32 ? 32 : 64);
    const int RPW = 64 / LPR;
    const int NQ = (mv + 63) / 64;
    const int grp = lane / LPR, col = lane - grp * LPR;
    const VT* Wv = reinterpret_cast<const VT*>(a.W);
    const VT* Wbv = reinterpret_cast<const VT*>(a.Wb);
    const int p0 = a.indptr[ex], p1 = a.indptr[ex + 1];
    VT acc[2];
    vzero(acc[0]);
    vzero(acc[1]);
    for (int pc = p0; pc < p1; pc += 64) {
        const int nf = min(64, p1 - pc);
        const int fid = lane < nf ? a.indices[pc + lane] : 0;
        const float fval = (lane < nf) ? (a.values ? a.values[pc + lane] : 1.f) : 0.f;
        for (int t0 = 0; t0 < nf; t0 += U * RPW) {
            VT x[U][2];
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * RPW + grp;
                const int tc = t < nf ? t : 0;
                const int f = __shfl(fid, tc, 64);       // on every lane (see k_label)
                const float fv = __shfl(fval, tc, 64);
                v[u] = t < nf ? fv : 0.f;
                const VT* row = Wv + (int64_t)f * mv;
                x[u][0] = row[col < mv ? col : 0];
                if (NQ > 1) x[u][1] = row[col + 64 < mv ? col + 64 : 0];
                else vzero(x[u][1]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < 2; ++q) vfma(acc[q], v[u], x[u][q]);
        }
    }
    lbl_fold<V4>(acc[0], RPW);
    // group 0 lanes hold S for columns col (+64): log-softmax, P, the entropy
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = col + 64 * q;
        const bool cv = grp == 0 && q < NQ && c < mv;
        VT sv = acc[q];
        if (cv) vadd(sv, Wbv[c]);
        acc[q] = sv;
        const float* se = reinterpret_cast<const float*>(&sv);
#pragma unroll
        for (int i = 0; i < VW; ++i)
            if (cv) mx = fmaxf(mx, se[i]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = col + 64 * q;
        if (grp == 0 && q < NQ && c < mv) {
            const float* sv = reinterpret_cast<const float*>(&acc[q]);
#pragma unroll
            for (int i = 0; i < VW; ++i) sum += expf(sv[i] - mx);
        }
    }
    sum = wave_sum(sum);
    const float lse = logf(sum);
    float h = 0.f;
    VT* pr = reinterpret_cast<VT*>(Pout);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = col + 64 * q;
        if (grp == 0 && q < NQ && c < mv) {
            VT o = acc[q];
            float* oe = reinterpret_cast<float*>(&o);
#pragma unroll
            for (int i = 0; i < VW; ++i) {
                const float lp = oe[i] - mx - lse;
                const float p = expf(lp);
                h += p * lp;
                oe[i] = p;
            }
            pr[c] = o;
        }
    }
    h = wave_sum(h);
    return -a.alpha * h;
}

// out[b][i] = sum_k P[b][k] C[i][k] for the tile's 16 examples, i < r (one wave per 16 rows i,
// job-strided over the workgroup's waves): D[i][b] on v_mfma_f32_16x16x4_f32, A = C rows
// (lane (li, g): C[i0 + li][k]), B = P^T from LDS (lane (li, g): P[li][k]); with m % 4 == 0 a
// lane's float4 of each feeds four instructions (k = k0 + 4g + q on both operands).
template <bool V4>
__device__ __forceinline__ void eval_project(const float* __restrict__ C, const float* sP, int mS,
                                             float* sOut, int RS, int m, int r, int it) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    const int i = it * 16 + li;
    const bool iv = i < r;
    const float* crow = C + (int64_t)(iv ? i : 0) * m;
    const float* prow = sP + li * mS;
    rae_ev4 acc = {0.f, 0.f, 0.f, 0.f};
    if (V4) {
        for (int k0 = 0; k0 < m; k0 += 16) {
            const int k = k0 + 4 * g;
            const bool ok = k < m;
            const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 cl = *reinterpret_cast<const float4*>(crow + (ok ? k : 0));
            const float4 pl = *reinterpret_cast<const float4*>(prow + (ok ? k : 0));
            const float4 ca = (ok && iv) ? cl : z4;
            const float4 pb = ok ? pl : z4;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.x, pb.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.y, pb.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.z, pb.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ca.w, pb.w, acc, 0, 0, 0);
        }
    } else {
        for (int k0 = 0; k0 < m; k0 += 4) {
            const int k = k0 + g;
            const bool ok = k < m;
            const float cl = crow[ok ? k : 0], pl = prow[ok ? k : 0];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32((ok && iv) ? cl : 0.f, ok ? pl : 0.f, acc,
                                                       0, 0, 0);
        }
    }
    // lane (li, g) holds D[i = 16 it + 4g + reg][b = li]
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int io = it * 16 + 4 * g + reg;
        if (io < r) sOut[li * RS + io] = acc[reg];
    }
}

// <row, vec> over r columns by one 16-lane group (sub = lane & 15); every lane of the group
// gets the identical sum.  row: global (an A row), vec: LDS.
__device__ __forceinline__ float eval_dot(const float* __restrict__ row, const float* vec, int r,
                                          int sub) {
    float acc = 0.f;
    if ((r & 3) == 0) {
        const float4* r4p = reinterpret_cast<const float4*>(row);
        const float4* v4p = reinterpret_cast<const float4*>(vec);
        const int rv = r >> 2;
#pragma unroll 4
        for (int c = sub; c < rv; c += 16) acc += vdot(r4p[c], v4p[c]);
    } else {
#pragma unroll 4
        for (int c = sub; c < r; c += 16) acc += row[c] * vec[c];
    }
    return group16_sum(acc);
}

// ---- k_eval_enc: RESCAL / hybrid encoder of the chunk ---------------------------------------
template <bool V4>
__device__ __forceinline__ void eval_enc(const EvalArgs& a) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nw = gridDim.x * RAE_EV_NW;
    for (int b = blockIdx.x * RAE_EV_NW + w; b < a.n; b += nw) {
        const float h = eval_encode<V4>(a, a.row0 + b, a.P + (int64_t)b * a.m);
        if (lane == 0) a.terms[(int64_t)b * 3 + 1] = h;
    }
}

// ---- k_eval_mt: partials of v = M a2 and w = M^T a1 ------------------------------------------
// four values of an A row at columns j .. j + 3 (zero past r or when !ok); j % 4 == 0
__device__ __forceinline__ float4 eval_row4(const float* __restrict__ row, int j, int r, bool ok) {
    float4 o;
    if ((r & 3) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(row + (j < r ? j : 0));
        const bool k = ok && j < r;
        o = make_float4(k ? v.x : 0.f, k ? v.y : 0.f, k ? v.z : 0.f, k ? v.w : 0.f);
    } else {
        const float x0 = row[j < r ? j : 0], x1 = row[j + 1 < r ? j + 1 : 0];
        const float x2 = row[j + 2 < r ? j + 2 : 0], x3 = row[j + 3 < r ? j + 3 : 0];
        o = make_float4((ok && j < r) ? x0 : 0.f, (ok && j + 1 < r) ? x1 : 0.f,
                        (ok && j + 2 < r) ? x2 : 0.f, (ok && j + 3 < r) ? x3 : 0.f);
    }
    return o;
}

// V4: m % 4 == 0 (float4 operands, four MFMAs each)
template <bool V4>
__device__ __forceinline__ void eval_mt(const EvalArgs& a, float* smem) {
    const int r = a.r, m = a.m, n = a.n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int nbj = eval_nbj(r);
    const int it = blockIdx.x / nbj, jt = blockIdx.x - it * nbj;
    const int i0 = it * RAE_EV_MTI, j0 = jt * RAE_EV_MTJ;
    // ---- stage: LDS row (ii, jj) = R[i0+ii][j0+jj][0..m); rows past r are zero
    if (V4) {
        const int m4 = m / 4, nv = RAE_EV_MTI * RAE_EV_MTJ * m4;
        for (int e = tid; e < nv; e += RAE_EV_MTT) {
            const int row = e / m4, kq = e - row * m4;
            const int i = i0 + row / RAE_EV_MTJ, j = j0 + row % RAE_EV_MTJ;
            const bool ok = i < r && j < r;
            const float4 x = *reinterpret_cast<const float4*>(
                a.R3 + ((int64_t)(ok ? i : 0) * r + (ok ? j : 0)) * m + 4 * kq);
            *reinterpret_cast<float4*>(smem + row * m + 4 * kq) =
                ok ? x : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        for (int e = tid; e < RAE_EV_MTI * RAE_EV_MTJ * m; e += RAE_EV_MTT) {
            const int row = e / m, k = e - row * m;
            const int i = i0 + row / RAE_EV_MTJ, j = j0 + row % RAE_EV_MTJ;
            smem[row * m + k] = (i < r && j < r) ? a.R3[((int64_t)i * r + j) * m + k] : 0.f;
        }
    }
    __syncthreads();
    const int nbt = (n + 15) / 16;
    for (int bt = w; bt < nbt; bt += RAE_EV_MTW) {
        const int bb = bt * 16 + li;
        const bool bv = bb < n;
        const int64_t ex = a.row0 + (bv ? bb : 0);
        const float* a1 = a.A + (int64_t)a.args1[ex] * r;
        const float* a2 = a.A + (int64_t)a.args2[ex] * r;
        const float* Pa = a.P + (int64_t)(bv ? bb : 0) * m;
        const float4 cv = eval_row4(a2, j0 + 4 * g, r, bv);       // contracted over j
        float cw[RAE_EV_MTI];                                     // contracted over i
#pragma unroll
        for (int q = 0; q < RAE_EV_MTI / 4; ++q) {
            const float4 c = eval_row4(a1, i0 + 4 * q, r, bv);
            cw[4 * q + 0] = c.x; cw[4 * q + 1] = c.y; cw[4 * q + 2] = c.z; cw[4 * q + 3] = c.w;
        }
        float vp[RAE_EV_MTI];
        float4 wacc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ii = 0; ii < RAE_EV_MTI; ++ii) {
            rae_ev4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* srow = smem + (ii * RAE_EV_MTJ + li) * m;
            if (V4) {
                for (int k0 = 0; k0 < m; k0 += 16) {
                    const int k = k0 + 4 * g;
                    const bool ok = k < m;
                    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 sl = *reinterpret_cast<const float4*>(srow + (ok ? k : 0));
                    const float4 pl = *reinterpret_cast<const float4*>(Pa + (ok ? k : 0));
                    const float4 sa = ok ? sl : z4;
                    const float4 pb = (ok && bv) ? pl : z4;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sa.x, pb.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sa.y, pb.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sa.z, pb.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sa.w, pb.w, acc, 0, 0, 0);
                }
            } else {
                for (int k0 = 0; k0 < m; k0 += 4) {
                    const int k = k0 + g;
                    const bool ok = k < m;
                    const float sl = srow[ok ? k : 0], pl = Pa[ok ? k : 0];
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? sl : 0.f, (ok && bv) ? pl : 0.f,
                                                               acc, 0, 0, 0);
                }
            }
            // lane (li, g): acc[reg] = M_b[i0 + ii][j0 + 4g + reg], b = bb
            vp[ii] = acc[0] * cv.x + acc[1] * cv.y + acc[2] * cv.z + acc[3] * cv.w;
            wacc.x += cw[ii] * acc[0];
            wacc.y += cw[ii] * acc[1];
            wacc.z += cw[ii] * acc[2];
            wacc.w += cw[ii] * acc[3];
        }
        // cv side: sum over the four lane groups (fixed order)
#pragma unroll
        for (int ii = 0; ii < RAE_EV_MTI; ++ii) {
            vp[ii] += __uint_as_float(xor16_u32(__float_as_uint(vp[ii])));
            vp[ii] += __uint_as_float(xor32_u32(__float_as_uint(vp[ii])));
        }
        if (bv) {
            if (4 * g < RAE_EV_MTI && i0 + 4 * g < r) {
                float4 o = make_float4(vp[0], vp[1], vp[2], vp[3]);
#pragma unroll
                for (int q = 1; q < RAE_EV_MTI / 4; ++q)
                    if (g == q) o = make_float4(vp[4 * q], vp[4 * q + 1], vp[4 * q + 2], vp[4 * q + 3]);
                *reinterpret_cast<float4*>(a.vpart + ((int64_t)jt * a.cap + bb) * a.r4 + i0 + 4 * g) = o;
            }
            if (j0 + 4 * g < r)
                *reinterpret_cast<float4*>(a.wpart + ((int64_t)it * a.cap + bb) * a.r4 + j0 + 4 * g) = wacc;
        }
    }
}

// ---- the tile's contraction vectors and positive scores (shared with rae_rank.hpp) ------------
// LDS of one tile of RAE_EV_TE examples (eval_dec_lds_floats)
struct EvalTile {
    float* sP;                                // the tile's P
    float* sL;                                // contracted with the neg1 rows (and a1)
    float* sR;                                // contracted with the neg2 rows
    float* sC1;                               // hybrid: wC1, wC2
    float* sC2;
};
__device__ __forceinline__ EvalTile eval_tile(const EvalArgs& a, float* sm) {
    const int mS = (a.m + 3) & ~3, r4 = a.r4;
    EvalTile t;
    t.sP = sm;
    t.sL = t.sP + RAE_EV_TE * mS;
    t.sR = t.sL + RAE_EV_TE * r4;
    t.sC1 = t.sR + RAE_EV_TE * r4;
    t.sC2 = t.sC1 + RAE_EV_TE * r4;
    return t;
}

// phases 1 - 2b of a tile: sL / sR (hybrid: sC1 / sC2 too) of the workgroup's RAE_EV_TE examples;
// ends on a barrier
template <bool V4>
__device__ __forceinline__ void eval_tile_vectors(const EvalArgs& a, const EvalTile& T) {
    const int m = a.m, r = a.r, dec = a.dec;
    const int mS = (m + 3) & ~3, r4 = a.r4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *sP = T.sP, *sL = T.sL, *sR = T.sR, *sC1 = T.sC1, *sC2 = T.sC2;
    const int tb = blockIdx.x * RAE_EV_TE;
    // ---- phase 1: the tile's P in LDS (SP: the encoder here; hybrid: from the workspace)
    if (dec != 1) {
        for (int q = w; q < RAE_EV_TE; q += RAE_EV_NW) {
            const int b = tb + q;
            if (b < a.n) {
                if (dec == 0) {
                    const float h = eval_encode<V4>(a, a.row0 + b, sP + q * mS);
                    if (lane == 0) a.terms[(int64_t)b * 3 + 1] = h;
                } else {
                    for (int k = lane; k < m; k += 64) sP[q * mS + k] = a.P[(int64_t)b * m + k];
                }
            } else {
                for (int k = lane; k < m; k += 64) sP[q * mS + k] = 0.f;
            }
        }
        __syncthreads();
        // ---- phase 2a: wC1 / wC2 = P.C^T of the tile
        const int nit = (r + 15) / 16;
        for (int job = w; job < 2 * nit; job += RAE_EV_NW) {
            const bool second = job >= nit;
            const int it = second ? job - nit : job;
            float* out = dec == 0 ? (second ? sR : sL) : (second ? sC2 : sC1);
            eval_project<V4>(second ? a.C2 : a.C1, sP, mS, out, r4, m, r, it);
        }
        __syncthreads();
    }
    // ---- phase 2b: v / w of the tile: the block partials in block order (+ wC1 / wC2)
    if (dec != 0) {
        const int nbi = eval_nbi(r), nbj = eval_nbj(r);
        for (int e = tid; e < RAE_EV_TE * r4; e += RAE_EV_BT) {
            const int q = e / r4, i = e - q * r4;
            const int b = tb + q;
            if (b < a.n && i < r) {
                float v = 0.f, wv = 0.f;
                const float* vq = a.vpart + (int64_t)b * r4 + i;
                const float* wq = a.wpart + (int64_t)b * r4 + i;
                const int64_t bs = (int64_t)a.cap * r4;
#pragma unroll 4
                for (int t = 0; t < nbj; ++t) v += vq[t * bs];
#pragma unroll 4
                for (int t = 0; t < nbi; ++t) wv += wq[t * bs];
                if (dec == 2) { v += sC1[e]; wv += sC2[e]; }
                sL[e] = v;
                sR[e] = wv;
            }
        }
        __syncthreads();
    }
}

// the positive dots of example slot q of the tile by one wave: one (the objective's positive
// score without the entity bias), addL (added to every neg1 score) and addR (to every neg2 score)
__device__ __forceinline__ void eval_positive(const EvalArgs& a, const EvalTile& T, int q, int e1,
                                              int e2, float& one, float& addL, float& addR) {
    const int r = a.r, r4 = a.r4, dec = a.dec;
    const int lane = threadIdx.x & 63;
    const int grp = lane >> 4, sub = lane & 15;
    const float *sC1 = T.sC1, *sC2 = T.sC2;
    const float* vL = T.sL + q * r4;
    const float* vR = T.sR + q * r4;
    // positives.  SP (A[args1] twice, the reference's behaviour): left = <wC1,a1>,
    // right = <wC2,a1>.  RESCAL: one = <a1, M a2>.  Hybrid: <a1, M a2 + wC1>, sp2 =
    // <wC2,a2>, sp1 = <wC1,a1>
    const int prow = (dec == 2 && grp == 1) ? e2 : e1;
    const float* pvec = dec == 0 ? (grp == 1 ? vR : vL)
                                 : (dec == 1 ? vL
                                             : (grp == 0 ? vL : (grp == 1 ? sC2 + q * r4
                                                                          : sC1 + q * r4)));
    const float pd = eval_dot(a.A + (int64_t)prow * r, pvec, r, sub);
    const float d0 = __shfl(pd, 0, 64), d1 = __shfl(pd, 16, 64), d2 = __shfl(pd, 32, 64);
    if (dec == 0) { one = d0 + d1; addL = d1; addR = d0; }
    else if (dec == 1) { one = d0; addL = 0.f; addR = 0.f; }
    else { one = d0 + d1; addL = d1; addR = d2; }
}

// ---- k_eval_dec: the tile's scores ------------------------------------------------------------
template <bool V4>
__device__ __forceinline__ void eval_dec(const EvalArgs& a, float* sm) {
    const int r = a.r, s = a.s, r4 = a.r4;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tb = blockIdx.x * RAE_EV_TE;
    const EvalTile T = eval_tile(a, sm);
    eval_tile_vectors<V4>(a, T);
    // ---- phase 3: per example (one wave each) the A-row gathers, four rows per instruction
    const int grp = lane >> 4, sub = lane & 15;
    for (int q = w; q < RAE_EV_TE; q += RAE_EV_NW) {
        const int b = tb + q;
        if (b >= a.n) continue;
        const int64_t ex = a.row0 + b;
        const int e1 = a.args1[ex], e2 = a.args2[ex];
        const float* vL = T.sL + q * r4;
        const float* vR = T.sR + q * r4;
        float one, addL, addR;
        eval_positive(a, T, q, e1, e2, one, addL, addR);
        const float pos = eval_logsig(one + a.Ab[e1]) + eval_logsig(one + a.Ab[e2]);
        // negatives: task t < s: neg1[t] against vL; s <= t < 2s: neg2[t - s] against vR
        float nacc = 0.f;
        // (two rounds of four rows per iteration: their gathers are in flight together)
        for (int t0 = 0; t0 < 2 * s; t0 += 8) {
            float d[2], add[2];
            bool valid[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = t0 + 4 * u + grp;
                valid[u] = t < 2 * s;
                const bool side = t >= s;
                const int tt = valid[u] ? (side ? t - s : t) : 0;
                const int32_t* np = side ? a.neg2 : a.neg1;
                const int id = np[(int64_t)tt * a.neg_stride + ex];
                d[u] = eval_dot(a.A + (int64_t)id * r, side ? vR : vL, r, sub);
                add[u] = (side ? addR : addL) + a.Ab[id];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float ls = eval_logsig(-(d[u] + add[u]));
                if (valid[u]) nacc += ls;
            }
        }
        const float n0 = __shfl(nacc, 0, 64), n1 = __shfl(nacc, 16, 64);
        const float n2 = __shfl(nacc, 32, 64), n3 = __shfl(nacc, 48, 64);
        if (lane == 0) {
            a.terms[(int64_t)b * 3 + 0] = pos;
            a.terms[(int64_t)b * 3 + 2] = (n0 + n1) + (n2 + n3);
        }
    }
}

// ---- the column sums ----------------------------------------------------------------------------
// partial[blk] = the three column sums of rows [1024 blk, 1024 (blk + 1)) of the chunk's terms,
// in double: thread t adds rows t, t + 256, ... in order, then the wave tree, then the waves in
// order
__device__ __forceinline__ void eval_blocksum(const float* __restrict__ terms, int n,
                                              double* __restrict__ partial, double* red) {
    const int tid = threadIdx.x, w = tid >> 6;
    double sacc[3] = {0.0, 0.0, 0.0};
    for (int u = 0; u < RAE_EV_SUMROWS / RAE_EV_BT; ++u) {
        const int row = blockIdx.x * RAE_EV_SUMROWS + u * RAE_EV_BT + tid;
        if (row < n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sacc[c] += (double)terms[(int64_t)row * 3 + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) sacc[c] = wave_sum_d(sacc[c]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) red[w * 3 + c] = sacc[c];
    }
    __syncthreads();
    if (tid < 3) {
        double t = red[tid];
#pragma unroll
        for (int i = 1; i < RAE_EV_NW; ++i) t += red[i * 3 + tid];
        partial[blockIdx.x * 3 + tid] = t;
    }
}

}  // namespace rae
