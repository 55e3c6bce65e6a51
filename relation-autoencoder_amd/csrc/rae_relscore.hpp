// rae_relation_scores / rae_eval_relations: the decoder's score of every relation for a pair of
// entities (no reference counterpart: the reference contracts the encoder's P into the decoder
// before the entities are touched, so psi_b. never exists there).
//   psi_k(e1, e2) = a1^T R[:,:,k] a2  (+ <C1[:,k], a1> + <C2[:,k], a1 or a2>),  a1 = A[e1], a2 = A[e2]
// is the GEMM  Psi = U . B  with
//   U_b[(i, j)] = a1_bi a2_bj   generated in registers, never stored,
//   B = R3 viewed as an (r^2 x m) row-major matrix (its memory layout already),
// and the SP terms as 2r further K rows: [a1 ; a1 (sp) or a2 (hybrid)] against [C1 ; C2].
// K = r^2 (rescal), 2r (sp), r^2 + 2r (hybrid).
//
// Kernels:
//   k_relscore   workgroup (example block, column group) of 8 waves.  A column group is NT =
//                NTA + NTB tiles of 16 relations; wave w owns the 16 examples of example tile
//                w % ET and the NTA (column split 0) or NTB (split 1) tiles of split w / ET, ET = 8
//                (NT = 1: 128 examples per workgroup) or 4 (64 examples).  (NTA, NTB) and the slab
//                depth TK are chosen from m alone (rel_config).  v_mfma_f32_16x16x4_f32 with the
//                relations on the rows (A operand: lane (li, g) reads a B row at column
//                16 ct + li from LDS) and the examples on the columns (B operand: lane (li, g)
//                holds u = a1[i] a2[j] of example li).  MFMA step s = 4 q + e of a slab contracts
//                the four K rows k0 + 16 q + 4 g + e, g = 0..3: a lane's K rows come in fours, so
//                its a2 values are float4 loads when r % 4 == 0 (a per-element gather otherwise),
//                64 consecutive bytes per example and instruction, with one a1 value per four.  The
//                accumulation order of a value is fixed by that mapping and by TK: by m alone.  NTA / NTB independent accumulator chains per wave, no branch inside
//                the MFMA loop.
//                B streams through LDS in slabs of TK K rows, double-buffered: the next slab's
//                global loads (and the next a1 / a2 values) are issued before the current slab's
//                MFMAs, stored to the other buffer (multiplied) after them, one barrier per slab.
//                The loader permutes the slab's rows so that step s reads LDS rows 4 s + g; LDS row
//                stride = the group's columns rounded up to 16 mod 64 floats, so the 4 x 16 lanes
//                of an operand read hit 64 banks.  LDS: 2 TK stride floats, at most 84 KiB
//                (m = 320).
//   k_rel_enc    one wave per row: logits S = x W + Wb (features in CSR order, one fp32 chain per
//                column), log-softmax  z_k - log sum exp z,  z = S - max S.
//   k_rel_fin    one wave per row: l_k = logsig(psi_k + Ab[e1]) + logsig(psi_k + Ab[e2]),
//                J_k = logsoftmax_k + l_k, the two argmaxes (k_label's rule).
// Determinism: there is no split-K.  One psi value is one accumulator of one MFMA chain over the
// slabs in ascending order; which lane or wave holds it does not enter its arithmetic, so it is a
// function of the pair's operands and of (decoder, r, m) alone.  No atomics.
#pragma once
#include "rae_common.hpp"
#include "rae_eval.hpp"
#include "rae_label.hpp"

namespace rae {

#define RAE_RS_BT 512             // threads per k_relscore workgroup
#define RAE_RS_NW (RAE_RS_BT / RAE_WAVE)
#define RAE_RS_TK 32              // K rows per LDS slab at least (rel_config: 32, 64 or 128)
#define RAE_RS_MAXNT 20           // column tiles per group at most (320 columns)
#define RAE_RS_ROUND 16384        // pairs / rows per launch round
#define RAE_RS_EBT 256            // threads per k_rel_enc / k_rel_fin workgroup
#define RAE_RS_MAXQ 8             // columns per lane of k_rel_enc / k_rel_fin (m <= 512)

typedef float rae_rs4 __attribute__((ext_vector_type(4)));

struct RelArgs {
    int dec, m, r;
    const float *A, *C1, *C2, *R3;
    const int32_t *e1, *e2;       // (nq) of the round
    int64_t n_ent;
    int nq;                       // pairs of the round (<= RAE_RS_ROUND)
    float* psi;                   // (nq, ldp) of the round
    int64_t ldp;
    int KR, K;                    // r^2 (0 for sp), the whole contraction length
    unsigned rinv;                // floor(2^32 / r) + 1 (r > 1): kk / r = umulhi(kk, rinv)
    int av4;                      // r % 4 == 0 and A 16-byte aligned: float4 loads of a2 runs
};

struct RelConfig { int nta, ntb, tk; };
// the tile configuration: a function of m alone.  NT = nta + ntb column tiles per group, the
// smallest of {1, 2, 4, 7, 8, 12, 16, 20} that holds the relations (20 and several groups above
// 320); deeper slabs where the group is narrow, so that a slab's MFMAs cover its loads' latency
__host__ __device__ inline RelConfig rel_config(int m) {
    const int nt = (m + 15) / 16;
    RelConfig c;
    if (nt <= 1) { c.nta = 1; c.ntb = 0; c.tk = 128; }
    else if (nt <= 2) { c.nta = 1; c.ntb = 1; c.tk = 64; }
    else if (nt <= 4) { c.nta = 2; c.ntb = 2; c.tk = 64; }
    else if (nt <= 7) { c.nta = 4; c.ntb = 3; c.tk = 64; }
    else if (nt <= 8) { c.nta = 4; c.ntb = 4; c.tk = 64; }
    else if (nt <= 12) { c.nta = 6; c.ntb = 6; c.tk = 32; }
    else if (nt <= 16) { c.nta = 8; c.ntb = 8; c.tk = 32; }
    else { c.nta = 10; c.ntb = 10; c.tk = 32; }
    return c;
}
__host__ __device__ constexpr int rel_ld(int wc) {       // LDS row stride: wc up to 16 mod 64
    return wc <= 16 ? 16 : ((wc - 16 + 63) / 64) * 64 + 16;
}
__host__ __device__ inline int rel_group_cols(RelConfig c) { return (c.nta + c.ntb) * 16; }
__host__ __device__ inline int rel_block_examples(RelConfig c) {
    return (RAE_RS_NW / (c.ntb > 0 ? 2 : 1)) * 16;
}
__host__ __device__ inline size_t rel_lds_bytes(RelConfig c) {
    return (size_t)2 * c.tk * rel_ld(rel_group_cols(c)) * sizeof(float);
}

// row kk of B (kk < K): R3 rows, then C1's, then C2's
__device__ __forceinline__ const float* rel_brow(const RelArgs& a, int kk) {
    if (kk < a.KR) return a.R3 + (int64_t)kk * a.m;
    const int t = kk - a.KR;
    if (t < a.r) return a.C1 + (int64_t)t * a.m;
    return a.C2 + (int64_t)(t - a.r) * a.m;
}

// N accumulator chains over one slab: step s contracts LDS rows 4 s + g with u[s]
template <int N, int NS, int LD, int NACC>
__device__ __forceinline__ void rel_mma(const float* bp, const float (&u)[NS],
                                        rae_rs4 (&acc)[NACC]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int ct = 0; ct < N; ++ct)
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(bp[4 * s * LD + ct * 16], u[s], acc[ct],
                                                           0, 0, 0);
    }
}

template <int NTA, int NTB, int TK>
__device__ __forceinline__ void rel_scores(const RelArgs& a, float* smem) {
    constexpr int CS = NTB > 0 ? 2 : 1;
    constexpr int ET = RAE_RS_NW / CS;
    constexpr int WC = (NTA + NTB) * 16;
    constexpr int LD = rel_ld(WC);
    constexpr int QPR = WC / 4;                           // float4 per slab row
    constexpr int NQD = TK * QPR;
    constexpr int PF = (NQD + RAE_RS_BT - 1) / RAE_RS_BT;
    constexpr int SLAB = TK * LD;
    constexpr int NS = TK / 4;                            // MFMA k steps per slab
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int et = w % ET, cs = w / ET;
    const int m = a.m, r = a.r, K = a.K, KR = a.KR;
    // groups wider than 128 columns only serve m > 128, where m % 4 == 0 is a shape rule
    const bool v4 = (NTA + NTB) > 8 || (m & 3) == 0;
    const int c0 = blockIdx.y * WC;                       // the group's first column
    const int cw = c0 + cs * NTA * 16;                    // the wave's first column
    const int b = blockIdx.x * (ET * 16) + et * 16 + li;
    const bool bv = b < a.nq;
    const int id1 = bv ? a.e1[b] : 0, id2 = bv ? a.e2[b] : 0;
    const unsigned nU = (unsigned)a.n_ent;
    const bool ok = (unsigned)id1 < nU && (unsigned)id2 < nU;
    const float* a1p = a.A + (int64_t)(ok ? id1 : 0) * r;
    const float* a2p = a.A + (int64_t)(ok ? id2 : 0) * r;
    const float* xp = a.dec == 0 ? a1p : a2p;             // against C2: sp keeps A[args1] twice

    // the factors of this lane's u at K rows k0 + 16 (s / 4) + 4 g + s % 4, s < NS:
    // u[s] = xq[s / 4] ya[s].  Fast form (the slab lies in the bilinear rows, r % 4 == 0: four
    // consecutive K rows at a multiple of 4 share their i): float4 loads of a2 -- the four lane
    // groups of an example read 64 consecutive bytes per instruction -- and one a1 value per
    // four, multiplied after the MFMAs.  Otherwise per element, multiplied at once (the loads are
    // then waited for before the MFMAs: r % 4 != 0, the SP rows, the last slab).
    auto load_u = [&](int k0, float (&xq)[NS / 4], float (&ya)[NS]) {
        if (a.av4 && k0 + TK <= KR) {                     // wave-uniform
#pragma unroll
            for (int q = 0; q < NS / 4; ++q) {
                const int kk = k0 + 16 * q + 4 * g;
                const int i = (int)__umulhi((unsigned)kk, a.rinv);
                const int j = kk - i * r;
                xq[q] = a1p[i];
                const float4 y = *reinterpret_cast<const float4*>(a2p + j);
                ya[4 * q + 0] = y.x; ya[4 * q + 1] = y.y; ya[4 * q + 2] = y.z; ya[4 * q + 3] = y.w;
            }
        } else {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int kk = k0 + 16 * (s >> 2) + 4 * g + (s & 3);
                const bool bil = kk < KR, sp = !bil && kk < K;
                const int i = r == 1 ? kk : (int)__umulhi((unsigned)kk, a.rinv);
                const int j = kk - i * r;
                const int t = kk - KR;
                const bool second = t >= r;
                const float* px = (sp && second) ? xp : a1p;
                const int ix = bil ? i : (sp ? (second ? t - r : t) : 0);
                const float x = px[ix];
                const float y = a2p[bil ? j : 0];
                ya[s] = bil ? x * y : (sp ? x : 0.f);
            }
#pragma unroll
            for (int q = 0; q < NS / 4; ++q) xq[q] = 1.f;
        }
    };
    float4 pf[PF];
    auto load_slab = [&](int k0) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int q = tid + p * RAE_RS_BT;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < NQD) {
                const int row = q / QPR, c4 = q - row * QPR;
                const int col = c0 + 4 * c4;
                const int kk = k0 + row;
                if (kk < K && col < m) {
                    const float* src = rel_brow(a, kk) + col;
                    if (v4) {
                        v = *reinterpret_cast<const float4*>(src);
                    } else {
                        v.x = src[0];
                        if (col + 1 < m) v.y = src[1];
                        if (col + 2 < m) v.z = src[2];
                        if (col + 3 < m) v.w = src[3];
                    }
                }
            }
            pf[p] = v;
        }
    };
    // slab row 16 q + 4 g + e (step s = 4 q + e of lane group g) goes to LDS row 4 s + g
    auto store_slab = [&](float* buf) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int q = tid + p * RAE_RS_BT;
            if (q < NQD) {
                const int row = q / QPR, c4 = q - row * QPR;
                const int lrow = (row & ~15) + 4 * (row & 3) + ((row >> 2) & 3);
                *reinterpret_cast<float4*>(buf + lrow * LD + 4 * c4) = pf[p];
            }
        }
    };

    rae_rs4 acc[NTA];
#pragma unroll
    for (int ct = 0; ct < NTA; ++ct) acc[ct] = rae_rs4{0.f, 0.f, 0.f, 0.f};
    float u[NS], xq[NS / 4], ya[NS];
    load_slab(0);
    load_u(0, xq, ya);
    store_slab(smem);
#pragma unroll
    for (int s = 0; s < NS; ++s) u[s] = xq[s / 4] * ya[s];
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < K; k0 += TK) {
        const bool more = k0 + TK < K;
        if (more) {
            load_slab(k0 + TK);
            load_u(k0 + TK, xq, ya);
        }
        const float* bp = smem + cur * SLAB + g * LD + (cs * NTA * 16 + li);
        if (NTB == 0 || cs == 0) rel_mma<NTA, NS, LD>(bp, u, acc);
        else rel_mma<(NTB > 0 ? NTB : 1), NS, LD>(bp, u, acc);
        if (more) {
            store_slab(smem + (cur ^ 1) * SLAB);
#pragma unroll
            for (int s = 0; s < NS; ++s) u[s] = xq[s / 4] * ya[s];
        }
        __syncthreads();                  // the other buffer is written, this one is read
        cur ^= 1;
    }
    // lane (li, g) holds psi[b][cw + 16 ct + 4 g + reg]
    if (bv) {
        float* out = a.psi + (int64_t)b * a.ldp;
        const float qnan = __uint_as_float(0x7fc00000u);
        const int cnt = cs == 0 ? NTA : NTB;
#pragma unroll
        for (int ct = 0; ct < NTA; ++ct) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int col = cw + 16 * ct + 4 * g + reg;
                if (ct < cnt && col < m) out[col] = ok ? acc[ct][reg] : qnan;
            }
        }
    }
}

// ---- k_rel_enc: the log-softmax of the encoder's logits -----------------------------------------
struct RelEnc {
    const int32_t *indptr, *indices;
    const float *values, *W, *Wb;
    int m;
    int64_t row0;
    int n;
    float* lsm;                   // (n, m)
};

__device__ __forceinline__ void rel_enc(const RelEnc& a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = a.m;
    const int nw = gridDim.x * (RAE_RS_EBT / RAE_WAVE);
    for (int b = blockIdx.x * (RAE_RS_EBT / RAE_WAVE) + w; b < a.n; b += nw) {
        const int64_t ex = a.row0 + b;
        const int p0 = a.indptr[ex], p1 = a.indptr[ex + 1];
        float acc[RAE_RS_MAXQ];
#pragma unroll
        for (int q = 0; q < RAE_RS_MAXQ; ++q) acc[q] = 0.f;
        for (int pc = p0; pc < p1; pc += 64) {
            const int nf = min(64, p1 - pc);
            const int fid = lane < nf ? a.indices[pc + lane] : 0;
            const float fval = lane < nf ? (a.values ? a.values[pc + lane] : 1.f) : 0.f;
            for (int t = 0; t < nf; ++t) {
                const int f = __shfl(fid, t, 64);
                const float fv = __shfl(fval, t, 64);
                const float* row = a.W + (int64_t)f * m;
#pragma unroll
                for (int q = 0; q < RAE_RS_MAXQ; ++q) {
                    const int c = lane + 64 * q;
                    if (c < m) acc[q] += fv * row[c];
                }
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < RAE_RS_MAXQ; ++q) {
            const int c = lane + 64 * q;
            if (c < m) {
                acc[q] += a.Wb[c];
                mx = fmaxf(mx, acc[q]);
            }
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < RAE_RS_MAXQ; ++q) {
            const int c = lane + 64 * q;
            if (c < m) {
                acc[q] -= mx;
                sum += expf(acc[q]);
            }
        }
        sum = wave_sum(sum);
        const float lse = logf(sum);
        float* out = a.lsm + (int64_t)b * m;
#pragma unroll
        for (int q = 0; q < RAE_RS_MAXQ; ++q) {
            const int c = lane + 64 * q;
            if (c < m) out[c] = acc[q] - lse;
        }
    }
}

// ---- k_rel_fin: J and the two labels ----------------------------------------------------------
struct RelFin {
    const float* psi; int64_t ldp;    // (n, ldp) of the round
    const float* lsm;                 // (n, m) or NULL (no joint output wanted)
    const float* Ab;
    const int32_t *e1, *e2;           // (n) of the round
    int64_t n_ent;
    int m, n;
    float* joint;                     // (n, m) or NULL
    int64_t *labels_dec, *labels_joint;   // (n) or NULL
};

__device__ __forceinline__ void rel_fin(const RelFin& a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = a.m;
    const int nw = gridDim.x * (RAE_RS_EBT / RAE_WAVE);
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int b = blockIdx.x * (RAE_RS_EBT / RAE_WAVE) + w; b < a.n; b += nw) {
        const int id1 = a.e1[b], id2 = a.e2[b];
        const unsigned nU = (unsigned)a.n_ent;
        const bool ok = (unsigned)id1 < nU && (unsigned)id2 < nU;
        const float b1 = ok ? a.Ab[id1] : qnan, b2 = ok ? a.Ab[id2] : qnan;
        const float* prow = a.psi + (int64_t)b * a.ldp;
        float bd = 0.f, bj = 0.f;
        int kd = 0x7fffffff, kj = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < RAE_RS_MAXQ; ++q) {
            const int c = lane + 64 * q;
            if (c < m) {
                const float p = prow[c];
                if (lbl_better(p, c, bd, kd)) { bd = p; kd = c; }
                if (a.lsm) {
                    const float l = eval_logsig(p + b1) + eval_logsig(p + b2);
                    const float J = a.lsm[(int64_t)b * m + c] + l;
                    if (a.joint) a.joint[(int64_t)b * m + c] = J;
                    if (lbl_better(J, c, bj, kj)) { bj = J; kj = c; }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(bd, o, 64), oj = __shfl_xor(bj, o, 64);
            const int okd = __shfl_xor(kd, o, 64), okj = __shfl_xor(kj, o, 64);
            if (lbl_better(od, okd, bd, kd)) { bd = od; kd = okd; }
            if (lbl_better(oj, okj, bj, kj)) { bj = oj; kj = okj; }
        }
        if (lane == 0) {
            if (a.labels_dec) a.labels_dec[b] = kd;
            if (a.labels_joint) a.labels_joint[b] = kj;
        }
    }
}

}  // namespace rae
