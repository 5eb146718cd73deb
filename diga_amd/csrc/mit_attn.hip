// Spatial-reduction attention of the MiT encoder (G5/model/networks/MixTransfomer.py:120-137): softmax(q k^T * scale) v with
// head_dim D = 64 (mit_b1..b5) or 32 (mit_b0; every kernel is a template on D, see "head width" below) and a short,
// spatially reduced key / value sequence (Nk = N / sr^2: 576 keys for every stage of a 768x768 crop).  Flash-style: scores
// never leave registers.  fp16 operands, fp32 accumulation (v_mfma_f32_16x16x32_f16), fp32 softmax in the log2 domain.
//
// Every product is formed TRANSPOSED so that the result of one MFMA is the B operand of the next without any lane
// movement: S^T = K Q^T has the key on the accumulator row (4 g + e, g = lane >> 4) and the query on the lane column, which
// is exactly the operand layout of  O^T = V^T P^T  once the k-slots (g, j) of that MFMA are read as
//   key(g, j) = 4 g + j (j < 4, first 16-key tile)   |   16 + 4 g + j - 4 (j >= 4, second tile)
// -- and V^T in that same key order is what the transposing ds_read_b64_tr_b16 delivers from a row-major [key][d] image
// (per 16-lane group a 4-row x 16-column block, lane i receiving column i).  Softmax reductions over keys run over a
// lane's 16 registers plus two cross-lane steps (lane ^ 16, lane ^ 32).
//
//   attn_fwd_kernel    O, LSE                 block = 8 waves x 32 queries, loop over 64-key blocks (K, V via LDS-DMA)
//   attn_bwd_dq_kernel dQ, delta = rowsum(dO*O)  same structure, recomputes P from LSE
//   attn_bwd_dkv_kernel dK, dV                block = 4 waves x 16 keys, loop over 64-query blocks (Q, dO via LDS-DMA),
//                                             query range split across blocks, fp32 slabs reduced in fixed order
//
// Head width.  D = 64: one key (query) per 128-byte LDS row, two k-halves per Q / K fragment, four d-tiles per output.  D = 32: the
// 64 bytes of TWO keys share one 128-byte LDS line (line = key >> 1, 16-byte chunks 4 (key & 1) .. + 3), so the line swizzle and
// the one-instruction LDS-DMA fill of 8 lines are the same code and a fill covers 16 keys; one k-fragment covers the head
// (k = 8 g + j), two d-tiles per output.  Bank argument for both widths: DESIGN.md section 9b.
#include "mit_common.h"

namespace diga {
namespace mit {

struct AttnArgs {
    const _Float16* Q;        // [B*N][ldq], head h at columns h*D..
    const _Float16* K;        // [B*Nk][ldkv]
    const _Float16* V;        // [B*Nk][ldkv]
    int64_t ldq, ldkv;
    _Float16* O;              // [B*N][ldo]           (forward: out; backward: saved forward output)
    int64_t ldo;
    float* lse;               // [B][heads][N], log2 domain
    const _Float16* dO;       // [B*N][ldo]
    _Float16* dQ;             // [B*N][ldq]
    float* delta;             // [B][heads][N]
    float* slab;              // dkv: [splits][B*Nk][2*heads*D] fp32
    int B, heads, N, Nk;
    int q_blocks;             // fwd / dq: blocks of 256 queries per (b, head)
    int k_blocks, splits, qblocks_per_split;   // dkv
    float scale, scale_log2e;
};

constexpr int kRowB = 128;                 // bytes per LDS line: 64 halves = one key of width 64 or two keys of width 32
template <int D>
constexpr int kImg = 64 * D * 2;           // one 64-key image: 8 KB (64 lines) at D = 64, 4 KB (32 lines) at D = 32

// LDS-DMA fill of 8 lines x 128 bytes (fill unit w8 = lines 8 w8 .. 8 w8 + 7 of an image: 8 keys at D = 64, 16 at D = 32) from rows
// (base + row * ld), rows clamped to [0, nrows).  One instruction: lane -> line l >> 3, destination chunk l & 7, source chunk
// swizzled; at D = 32 the logical chunk c of a line holds chunk c & 3 of key 2 line + (c >> 2).
template <int D>
__device__ __forceinline__ void fill_rows8(const _Float16* base, int64_t ld, int row0, int nrows, unsigned char* img, int w8, int lane) {
    const int r = 8 * w8 + (lane >> 3);
    const int chunk = (lane & 7) ^ swz128(r);
    if constexpr (D == 64) {
        const int src_row = min(row0 + r, nrows - 1);
        glds16(reinterpret_cast<const unsigned char*>(base + (int64_t)src_row * ld) + chunk * 16, img + (8 * w8) * kRowB);
    } else {
        const int src_row = min(row0 + 2 * r + (chunk >> 2), nrows - 1);
        glds16(reinterpret_cast<const unsigned char*>(base + (int64_t)src_row * ld) + (chunk & 3) * 16, img + (8 * w8) * kRowB);
    }
}

// row-wise (ds_read_b128) fragment of a 16-row tile: row = lane & 15, k = 32 half + 8 (lane >> 4) + j  (D = 32: half = 0)
template <int D>
__device__ __forceinline__ f16x8 row_frag(const unsigned char* img, int tile, int half, int lane) {
    const int r = 16 * tile + (lane & 15);
    if constexpr (D == 64) {
        const int chunk = 4 * half + (lane >> 4);
        return *reinterpret_cast<const f16x8*>(img + r * kRowB + ((chunk ^ swz128(r)) << 4));
    } else {
        const int line = r >> 1, chunk = 4 * (r & 1) + (lane >> 4);
        return *reinterpret_cast<const f16x8*>(img + line * kRowB + ((chunk ^ swz128(line)) << 4));
    }
}

// transposed fragment: element j of lane (g, i) = img[32 kk + (j < 4 ? 4 g + j : 16 + 4 g + j - 4)][16 dt + i]
template <int D>
__device__ __forceinline__ f16x8 col_frag(const unsigned char* img, int kk, int dt, int lane) {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int r0 = 32 * kk + 4 * g + q, r1 = r0 + 16;
    if constexpr (D == 64) {
        const int chunk = 2 * dt + (pp >> 1);
        return tr_frag(img + r0 * kRowB + ((chunk ^ swz128(r0)) << 4) + ((pp & 1) << 3),
                       img + r1 * kRowB + ((chunk ^ swz128(r1)) << 4) + ((pp & 1) << 3));
    } else {
        const int l0 = r0 >> 1, l1 = r1 >> 1;                  // r1 = r0 + 16: the same half of line l0 + 8
        const int chunk = 4 * (r0 & 1) + 2 * dt + (pp >> 1);
        return tr_frag(img + l0 * kRowB + ((chunk ^ swz128(l0)) << 4) + ((pp & 1) << 3),
                       img + l1 * kRowB + ((chunk ^ swz128(l1)) << 4) + ((pp & 1) << 3));
    }
}

// The K and V (forward, dQ: 8 waves) images of one 64-key block.  D = 64: every wave fills unit w of both (2 instructions per wave
// and block); D = 32: an image is 4 units, waves 0..3 fill K and waves 4..7 fill V (1 instruction).  kKvFills is what the
// s_waitcnt vmcnt(N) behind the NEXT block's issue leaves in flight.
template <int D>
constexpr int kKvFills = D / 32;
template <int D>
__device__ __forceinline__ void fill_kv(const _Float16* Kb, const _Float16* Vb, int64_t ld, int row0, int nrows, unsigned char* base, int wv, int lane) {
    if constexpr (D == 64) {
        fill_rows8<64>(Kb, ld, row0, nrows, base, wv, lane);
        fill_rows8<64>(Vb, ld, row0, nrows, base + kImg<64>, wv, lane);
    } else {
        fill_rows8<32>(wv < 4 ? Kb : Vb, ld, row0, nrows, wv < 4 ? base : base + kImg<32>, wv & 3, lane);
    }
}
template <int D>
__device__ __forceinline__ void wait_kv_fills(bool ahead) {
    if (!ahead) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (kKvFills<D> == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
}

// exp2 as ONE v_exp_f32: exp2f() wraps the instruction in a denormal-range rescue (compare, select, ldexp: five instructions per
// element, 34 v_exp_f32 + 36 v_ldexp_f32 + 57 v_cmp + 104 v_cndmask per key block in the forward) for results below 2^-126 -- which
// vanish in every sum and fp16 cast they enter here
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ f16x8 pack8(const f32x4& a, const f32x4& b) {
    return (f16x8){(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3], (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
}

// reductions over the four 16-lane groups of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48) with the VALU lane swaps of gfx950
// (v_permlane32_swap / v_permlane16_swap: no LDS round trip on the softmax's critical path): swapping a register with itself
// leaves {lower half twice, upper half twice} resp. {even rows twice, odd rows twice} in the two results
__device__ __forceinline__ float group_max(float v) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float group_sum(float v) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
template <int D, int QT>
__global__ __launch_bounds__(512) void attn_fwd_kernel(AttnArgs a) {
    constexpr int KH = D / 32, DT = D / 16;                        // k-halves of a Q / K fragment, d-tiles of the output
    extern __shared__ __align__(16) unsigned char smem[];          // 2 buffers x (K image + V image)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    int blk = xcd_remap(blockIdx.x, gridDim.x);            // the query blocks of one (image, head) share its K / V through one L2
    const int qb = blk % a.q_blocks;
    blk /= a.q_blocks;
    const int h = blk % a.heads, b = blk / a.heads;
    const int q0 = qb * (128 * QT) + wv * (16 * QT);
    const _Float16* Kb = a.K + (int64_t)b * a.Nk * a.ldkv + h * D;
    const _Float16* Vb = a.V + (int64_t)b * a.Nk * a.ldkv + h * D;
    const int nkb = (a.Nk + 63) / 64;

    auto issue = [&](int kb, int buf) { fill_kv<D>(Kb, Vb, a.ldkv, kb * 64, a.Nk, smem + buf * 2 * kImg<D>, wv, lane); };
    issue(0, 0);

    f16x8 qf[QT][KH];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int q = min(q0 + 16 * t + li, a.N - 1);
        const _Float16* qp = a.Q + ((int64_t)b * a.N + q) * a.ldq + h * D + 8 * g;
#pragma unroll
        for (int hf = 0; hf < KH; ++hf) qf[t][hf] = *reinterpret_cast<const f16x8*>(qp + 32 * hf);
    }
    f32x4 o[DT][QT];
    float m[QT], l[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        m[t] = -1e30f;
        l[t] = 0.f;
#pragma unroll
        for (int d = 0; d < DT; ++d) o[d][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    for (int kb = 0; kb < nkb; ++kb) {
        const bool ahead = kb + 1 < nkb;
        if (ahead) issue(kb + 1, (kb + 1) & 1);
        wait_kv_fills<D>(ahead);                               // the next block's fills stay in flight
        __builtin_amdgcn_s_barrier();
        const unsigned char* Ki = smem + (kb & 1) * 2 * kImg<D>;
        const unsigned char* Vi = Ki + kImg<D>;
        f32x4 s[4][QT];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f16x8 kf[KH];
#pragma unroll
            for (int hf = 0; hf < KH; ++hf) kf[hf] = row_frag<D>(Ki, kt, hf, lane);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int hf = 0; hf < KH; ++hf) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[hf], qf[t][hf], acc, 0, 0, 0);
                s[kt][t] = acc;
            }
        }
        if (kb * 64 + 64 > a.Nk) {                             // last key block of a ragged sequence (uniform branch): keys past Nk
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int t = 0; t < QT; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (kb * 64 + 16 * kt + 4 * g + e >= a.Nk) s[kt][t][e] = -1e30f;
        }
        f16x8 pf[QT][2];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            // m tracks the RAW score maximum (scale > 0); p = exp2(scale_log2e * (s - m)) as one fma per element
            float bm = -1e30f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int e = 0; e < 4; ++e) bm = fmaxf(bm, s[kt][t][e]);
            bm = group_max(bm);
            const float mn = fmaxf(m[t], bm);
            if (__any(mn > m[t])) {                                 // wave-uniform: the running maximum rarely moves after the first blocks
                const float alpha = exp2f((m[t] - mn) * a.scale_log2e);
                l[t] *= alpha;
#pragma unroll
                for (int d = 0; d < DT; ++d)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[d][t][e] *= alpha;
                m[t] = mn;
            }
            const float off = -mn * a.scale_log2e;
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = fast_exp2(fmaf(s[kt][t][e], a.scale_log2e, off));
                    s[kt][t][e] = p;
                    ps += p;
                }
            l[t] += ps;
            pf[t][0] = pack8(s[0][t], s[1][t]);
            pf[t][1] = pack8(s[2][t], s[3][t]);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const f16x8 vt = col_frag<D>(Vi, kk, d, lane);
#pragma unroll
                for (int t = 0; t < QT; ++t) o[d][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vt, pf[t][kk], o[d][t], 0, 0, 0);
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                       // everyone is done reading before the buffer is refilled
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const float lt = group_sum(l[t]);
        const float inv = 1.f / lt;
        const int q = q0 + 16 * t + li;
        if (q < a.N) {
            _Float16* op = a.O + ((int64_t)b * a.N + q) * a.ldo + h * D + 4 * g;
#pragma unroll
            for (int d = 0; d < DT; ++d)
                *reinterpret_cast<f16x4*>(op + 16 * d) = (f16x4){(_Float16)(o[d][t][0] * inv), (_Float16)(o[d][t][1] * inv),
                                                                 (_Float16)(o[d][t][2] * inv), (_Float16)(o[d][t][3] * inv)};
            if (g == 0 && a.lse != nullptr) a.lse[((int64_t)b * a.heads + h) * a.N + q] = m[t] * a.scale_log2e + log2f(lt);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// backward, dQ:  P^T = exp2(S^T c - lse), dP^T = V dO^T, dS^T = P^T (dP^T - delta) scale, dQ^T += K^T dS^T
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(512) void attn_bwd_dq_kernel(AttnArgs a) {
    constexpr int QT = 2, KH = D / 32, DT = D / 16;
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    int blk = xcd_remap(blockIdx.x, gridDim.x);            // the query blocks of one (image, head) share its K / V through one L2
    const int qb = blk % a.q_blocks;
    blk /= a.q_blocks;
    const int h = blk % a.heads, b = blk / a.heads;
    const int q0 = qb * 256 + wv * 32;
    const _Float16* Kb = a.K + (int64_t)b * a.Nk * a.ldkv + h * D;
    const _Float16* Vb = a.V + (int64_t)b * a.Nk * a.ldkv + h * D;
    const int nkb = (a.Nk + 63) / 64;
    auto issue = [&](int kb, int buf) { fill_kv<D>(Kb, Vb, a.ldkv, kb * 64, a.Nk, smem + buf * 2 * kImg<D>, wv, lane); };
    issue(0, 0);

    f16x8 qf[QT][KH], df[QT][KH];
    float lse[QT], delta[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int q = min(q0 + 16 * t + li, a.N - 1);
        const int64_t row = (int64_t)b * a.N + q;
        const _Float16* qp = a.Q + row * a.ldq + h * D + 8 * g;
        const _Float16* dp = a.dO + row * a.ldo + h * D + 8 * g;
        const _Float16* op = a.O + row * a.ldo + h * D + 8 * g;
        f16x8 of[KH];
#pragma unroll
        for (int hf = 0; hf < KH; ++hf) qf[t][hf] = *reinterpret_cast<const f16x8*>(qp + 32 * hf);
#pragma unroll
        for (int hf = 0; hf < KH; ++hf) df[t][hf] = *reinterpret_cast<const f16x8*>(dp + 32 * hf);
#pragma unroll
        for (int hf = 0; hf < KH; ++hf) of[hf] = *reinterpret_cast<const f16x8*>(op + 32 * hf);
        float dsum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (KH == 2) dsum += (float)df[t][0][e] * (float)of[0][e] + (float)df[t][1][e] * (float)of[1][e];
            else dsum += (float)df[t][0][e] * (float)of[0][e];
        }
        delta[t] = group_sum(dsum);
        lse[t] = a.lse[((int64_t)b * a.heads + h) * a.N + q];
        if (g == 0 && q0 + 16 * t + li < a.N) a.delta[((int64_t)b * a.heads + h) * a.N + q] = delta[t];
    }
    f32x4 dq[DT][QT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int d = 0; d < DT; ++d) dq[d][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < nkb; ++kb) {
        const bool ahead = kb + 1 < nkb;
        if (ahead) issue(kb + 1, (kb + 1) & 1);
        wait_kv_fills<D>(ahead);
        __builtin_amdgcn_s_barrier();
        const unsigned char* Ki = smem + (kb & 1) * 2 * kImg<D>;
        const unsigned char* Vi = Ki + kImg<D>;
        const bool tail = kb * 64 + 64 > a.Nk;
        f16x8 dsf[QT][2];
        f32x4 ds[4][QT];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f16x8 kf[KH], vf[KH];
#pragma unroll
            for (int hf = 0; hf < KH; ++hf) kf[hf] = row_frag<D>(Ki, kt, hf, lane);
#pragma unroll
            for (int hf = 0; hf < KH; ++hf) vf[hf] = row_frag<D>(Vi, kt, hf, lane);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                f32x4 sa = (f32x4){0.f, 0.f, 0.f, 0.f}, pa = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int hf = 0; hf < KH; ++hf) sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[hf], qf[t][hf], sa, 0, 0, 0);
#pragma unroll
                for (int hf = 0; hf < KH; ++hf) pa = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[hf], df[t][hf], pa, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = fast_exp2(sa[e] * a.scale_log2e - lse[t]);
                    ds[kt][t][e] = p * (pa[e] - delta[t]) * a.scale;
                }
            }
        }
        if (tail) {                                            // (uniform branch) keys past Nk: clamped copies of the last key
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int t = 0; t < QT; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (kb * 64 + 16 * kt + 4 * g + e >= a.Nk) ds[kt][t][e] = 0.f;
        }
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            dsf[t][0] = pack8(ds[0][t], ds[1][t]);
            dsf[t][1] = pack8(ds[2][t], ds[3][t]);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const f16x8 kt_ = col_frag<D>(Ki, kk, d, lane);
#pragma unroll
                for (int t = 0; t < QT; ++t) dq[d][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kt_, dsf[t][kk], dq[d][t], 0, 0, 0);
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int q = q0 + 16 * t + li;
        if (q < a.N) {
            _Float16* op = a.dQ + ((int64_t)b * a.N + q) * a.ldq + h * D + 4 * g;
#pragma unroll
            for (int d = 0; d < DT; ++d)
                *reinterpret_cast<f16x4*>(op + 16 * d) = (f16x4){(_Float16)dq[d][t][0], (_Float16)dq[d][t][1], (_Float16)dq[d][t][2], (_Float16)dq[d][t][3]};
        }
    }
}

// ---------------------------------------------------------------------------------------------
// backward, dK / dV: the block owns 64 keys (16 per wave), walks its range of 64-query blocks.
//   S = Q K^T (row = query 4 g + e, col = key), P = exp2(S c - lse_q), dP = dO V^T, dS = P (dP - delta_q) scale
//   dV += P^T dO, dK += dS^T Q: P / dS tiles are the A operands as they stand (k-slots = queries), dO / Q come transposed
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(AttnArgs a) {
    constexpr int KH = D / 32, DT = D / 16;
    extern __shared__ __align__(16) unsigned char smem[];          // 2 buffers x (Q image + dO image) + statistics
    float* stat = reinterpret_cast<float*>(smem + 4 * kImg<D>);    // [2 buffers][4 waves][64]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    int blk = xcd_remap(blockIdx.x, gridDim.x);            // the key blocks of one (image, head, query range) re-read the same Q / dO
    const int kblk = blk % a.k_blocks;
    blk /= a.k_blocks;
    const int split = blk % a.splits;
    blk /= a.splits;
    const int h = blk % a.heads, b = blk / a.heads;
    const int key = min(kblk * 64 + wv * 16 + li, a.Nk - 1);
    const _Float16* kp = a.K + ((int64_t)b * a.Nk + key) * a.ldkv + h * D + 8 * g;
    const _Float16* vp = a.V + ((int64_t)b * a.Nk + key) * a.ldkv + h * D + 8 * g;
    f16x8 kf[KH], vf[KH];
#pragma unroll
    for (int hf = 0; hf < KH; ++hf) {
        kf[hf] = *reinterpret_cast<const f16x8*>(kp + 32 * hf);
        vf[hf] = *reinterpret_cast<const f16x8*>(vp + 32 * hf);
    }
    const _Float16* Qb = a.Q + (int64_t)b * a.N * a.ldq + h * D;
    const _Float16* Db = a.dO + (int64_t)b * a.N * a.ldo + h * D;
    const float* lse_b = a.lse + ((int64_t)b * a.heads + h) * a.N;
    const float* del_b = a.delta + ((int64_t)b * a.heads + h) * a.N;
    const int nqb_total = (a.N + 63) / 64;
    const int qb0 = split * a.qblocks_per_split;
    const int qb1 = min(qb0 + a.qblocks_per_split, nqb_total);

    // per block and wave 5 (D = 64) / 3 (D = 32) LDS-DMA instructions: rows 16 w .. 16 w + 15 of the Q and dO images (2 + 2 fills
    // of 8 rows, resp. 1 + 1 of 16) and one 4-byte-wide one for the statistics of those 16 queries: stat[buf][w][0..15] = lse,
    // [16..31] = delta (lanes 32..63 fetch a dummy)
    auto issue = [&](int qb, int buf) {
        unsigned char* base = smem + buf * 2 * kImg<D>;
        if constexpr (D == 64) {
            fill_rows8<64>(Qb, a.ldq, qb * 64, a.N, base, 2 * wv, lane);
            fill_rows8<64>(Qb, a.ldq, qb * 64, a.N, base, 2 * wv + 1, lane);
            fill_rows8<64>(Db, a.ldo, qb * 64, a.N, base + kImg<64>, 2 * wv, lane);
            fill_rows8<64>(Db, a.ldo, qb * 64, a.N, base + kImg<64>, 2 * wv + 1, lane);
        } else {
            fill_rows8<32>(Qb, a.ldq, qb * 64, a.N, base, wv, lane);
            fill_rows8<32>(Db, a.ldo, qb * 64, a.N, base + kImg<32>, wv, lane);
        }
        const int q = min(qb * 64 + 16 * wv + (lane & 15), a.N - 1);
        const float* src = (lane & 16) ? del_b + q : lse_b + q;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(stat + buf * 256 + wv * 64), 4, 0, 0);
    };

    f32x4 dk[DT], dv[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        dk[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
        dv[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (qb0 < qb1) issue(qb0, 0);
    for (int qb = qb0; qb < qb1; ++qb) {
        const int buf = (qb - qb0) & 1;
        const bool ahead = qb + 1 < qb1;
        if (ahead) issue(qb + 1, buf ^ 1);
        if (!ahead) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if constexpr (D == 64) asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); // the next block's 5 LDS-DMA loads stay in flight
        else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");                         // (3 at D = 32)
        __builtin_amdgcn_s_barrier();
        const unsigned char* Qi = smem + buf * 2 * kImg<D>;
        const unsigned char* Di = Qi + kImg<D>;
        const float* sl = stat + buf * 256;
        const bool qtail = qb * 64 + 64 > a.N;
        f32x4 p[4], ds[4];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            f32x4 sa = (f32x4){0.f, 0.f, 0.f, 0.f}, pa = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int hf = 0; hf < KH; ++hf) sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(row_frag<D>(Qi, qt, hf, lane), kf[hf], sa, 0, 0, 0);
#pragma unroll
            for (int hf = 0; hf < KH; ++hf) pa = __builtin_amdgcn_mfma_f32_16x16x32_f16(row_frag<D>(Di, qt, hf, lane), vf[hf], pa, 0, 0, 0);
            const float4 l4 = *reinterpret_cast<const float4*>(sl + 64 * qt + 4 * g);
            const float4 d4 = *reinterpret_cast<const float4*>(sl + 64 * qt + 16 + 4 * g);
            const float le[4] = {l4.x, l4.y, l4.z, l4.w}, de[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pe = fast_exp2(sa[e] * a.scale_log2e - le[e]);
                p[qt][e] = pe;
                ds[qt][e] = pe * (pa[e] - de[e]) * a.scale;
            }
        }
        if (qtail) {                                           // (uniform branch) rows past N were filled with a clamped query
#pragma unroll
            for (int qt = 0; qt < 4; ++qt)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (qb * 64 + 16 * qt + 4 * g + e >= a.N) p[qt][e] = ds[qt][e] = 0.f;
        }
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
            const f16x8 pf = pack8(p[2 * qq], p[2 * qq + 1]);
            const f16x8 sf = pack8(ds[2 * qq], ds[2 * qq + 1]);
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                dv[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, col_frag<D>(Di, qq, d, lane), dv[d], 0, 0, 0);
                dk[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sf, col_frag<D>(Qi, qq, d, lane), dk[d], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    // slab[split][b*Nk + key][two*C + h*D + d]: rows = keys 4 g + e of this wave's 16, cols = d = 16 dt + li
    const int C2 = 2 * a.heads * D;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int kq = kblk * 64 + wv * 16 + 4 * g + e;
        if (kq >= a.Nk) continue;
        float* row = a.slab + ((int64_t)split * a.B * a.Nk + (int64_t)b * a.Nk + kq) * C2 + h * D + li;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            row[16 * d] = dk[d][e];
            row[a.heads * D + 16 * d] = dv[d][e];
        }
    }
}

__global__ __launch_bounds__(256) void dkv_reduce_kernel(const float* __restrict__ slab, _Float16* __restrict__ dkv, int64_t n4, int splits) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 s = reinterpret_cast<const float4*>(slab)[i];
        for (int k = 1; k < splits; ++k) {
            const float4 v = reinterpret_cast<const float4*>(slab)[(int64_t)k * n4 + i];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        reinterpret_cast<f16x4*>(dkv)[i] = (f16x4){(_Float16)s.x, (_Float16)s.y, (_Float16)s.z, (_Float16)s.w};
    }
}

}  // namespace mit
}  // namespace diga

using namespace diga;
using namespace diga::mit;

static int attn_check(const char* who, const void* q, const void* kv, int64_t B, int64_t heads, int64_t D, int64_t N, int64_t Nk, int64_t ldq,
                      int64_t ldkv, int64_t ldo) {
    DIGA_REQUIRE(D == 32 || D == 64, DIGA_EINVAL, "%s: head_dim %lld is not built (32 and 64 are)", who, (long long)D);
    DIGA_REQUIRE(q && kv && B > 0 && heads > 0 && N > 0 && Nk > 0, DIGA_EINVAL, "%s: null pointer / empty shape", who);
    DIGA_REQUIRE(ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 8 == 0 && ldq >= heads * D && ldkv >= 2 * heads * D && ldo >= heads * D, DIGA_EINVAL,
                 "%s: head_dim is %lld; leading dimensions must be multiples of 8 and hold all heads", who, (long long)D);
    DIGA_REQUIRE(aligned16(q) && aligned16(kv), DIGA_EALIGN, "%s: operands must be 16-byte aligned", who);
    DIGA_REQUIRE(B * N < (1ll << 31) && B * Nk < (1ll << 31), DIGA_EINVAL, "%s: too many tokens", who);
    return DIGA_OK;
}

namespace {
template <int D>
void launch_fwd(const AttnArgs& a, hipStream_t st) {
    // 32 queries per wave (D = 64: 124 VGPRs, two blocks per CU).  A 64-query variant (K / V fragments read from LDS once per 64
    // MFMAs, 209 VGPRs, one block per CU) measured 15-25 % SLOWER on every MiT-B5 stage (tools/bench_mit_ops.py --cold: 245 vs
    // 207 us on stage 1): the softmax's latency needs the second resident block.  (At D = 32 the 64-query variant was not built.)
    hipLaunchKernelGGL((attn_fwd_kernel<D, 2>), dim3((unsigned)(a.B * a.heads * a.q_blocks)), dim3(512), 4 * kImg<D>, st, a);
}
template <int D>
void launch_bwd(const AttnArgs& a, _Float16* dkv, hipStream_t st) {
    hipLaunchKernelGGL(attn_bwd_dq_kernel<D>, dim3((unsigned)(a.B * a.heads * a.q_blocks)), dim3(512), 4 * kImg<D>, st, a);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<D>, dim3((unsigned)(a.B * a.heads * a.splits * a.k_blocks)), dim3(256),
                       4 * kImg<D> + 2 * 256 * sizeof(float), st, a);
    const int64_t n4 = (int64_t)a.B * a.Nk * 2 * a.heads * D / 4;
    int64_t grid = ceil_div(n4, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(dkv_reduce_kernel, dim3((unsigned)grid), dim3(256), 0, st, a.slab, dkv, n4, a.splits);
}

struct DkvPlan {
    int k_blocks, splits, qblocks_per_split;
    size_t slab_bytes;                                     // [splits][B*Nk][2*heads*D] fp32
};
DkvPlan dkv_plan(int64_t B, int64_t heads, int64_t D, int64_t N, int64_t Nk) {
    DkvPlan p;
    p.k_blocks = (int)ceil_div(Nk, 64);
    const int64_t nqb = ceil_div(N, 64);
    int64_t splits = ceil_div(1024, B * heads * p.k_blocks);
    if (splits > ceil_div(nqb, 4)) splits = ceil_div(nqb, 4);
    if (splits < 1) splits = 1;
    p.qblocks_per_split = (int)ceil_div(nqb, splits);
    p.splits = (int)ceil_div(nqb, p.qblocks_per_split);
    p.slab_bytes = (size_t)p.splits * (size_t)B * (size_t)Nk * 2 * (size_t)heads * (size_t)D * sizeof(float);
    return p;
}
}  // namespace

/* q [B*N][ldq] (head h at columns D h..), kv [B*Nk][ldkv] (K at columns D h.., V at heads*D + D h..): the layouts the q / kv
 * Linear layers produce (MixTransfomer.py:122,130-132).  out [B*N][ldo], lse [B][heads][N] (nullable). */
extern "C" int diga_mit_attention_hd_fwd(const void* q, int64_t ldq, const void* kv, int64_t ldkv, void* out, int64_t ldo, float* lse,
                                         int64_t B, int64_t heads, int64_t head_dim, int64_t N, int64_t Nk, float scale, void* stream) {
    int rc = attn_check("mit_attention_fwd", q, kv, B, heads, head_dim, N, Nk, ldq, ldkv, ldo);
    if (rc) return rc;
    DIGA_REQUIRE(out && aligned16(out), DIGA_EINVAL, "mit_attention_fwd: out");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AttnArgs a{};
    a.Q = static_cast<const _Float16*>(q); a.K = static_cast<const _Float16*>(kv); a.V = a.K + heads * head_dim;
    a.ldq = ldq; a.ldkv = ldkv; a.O = static_cast<_Float16*>(out); a.ldo = ldo; a.lse = lse;
    a.B = (int)B; a.heads = (int)heads; a.N = (int)N; a.Nk = (int)Nk;
    a.scale = scale; a.scale_log2e = scale * 1.4426950408889634f;
    ProfScope prof(DIGA_PROF_MIT_ATTN_FWD, st, 4.0 * (double)B * heads * (double)N * (double)Nk * (double)head_dim);
    a.q_blocks = (int)ceil_div(N, 256);
    if (head_dim == 64) launch_fwd<64>(a, st);
    else launch_fwd<32>(a, st);
    return launch_status("mit_attention_fwd");
}

extern "C" int diga_mit_attention_fwd(const void* q, int64_t ldq, const void* kv, int64_t ldkv, void* out, int64_t ldo, float* lse,
                                      int64_t B, int64_t heads, int64_t N, int64_t Nk, float scale, void* stream) {
    return diga_mit_attention_hd_fwd(q, ldq, kv, ldkv, out, ldo, lse, B, heads, 64, N, Nk, scale, stream);
}

extern "C" size_t diga_mit_attention_hd_bwd_workspace_bytes(int64_t B, int64_t heads, int64_t head_dim, int64_t N, int64_t Nk) {
    if (B <= 0 || heads <= 0 || N <= 0 || Nk <= 0 || (head_dim != 32 && head_dim != 64)) return 0;
    return dkv_plan(B, heads, head_dim, N, Nk).slab_bytes + (size_t)B * heads * N * sizeof(float);
}

extern "C" size_t diga_mit_attention_bwd_workspace_bytes(int64_t B, int64_t heads, int64_t N, int64_t Nk) {
    return diga_mit_attention_hd_bwd_workspace_bytes(B, heads, 64, N, Nk);
}

/* Gradients of diga_mit_attention_hd_fwd: d_out [B*N][ldo] -> dq [B*N][ldq], dkv [B*Nk][ldkv] (same column layout as kv). */
extern "C" int diga_mit_attention_hd_bwd(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const void* out, const void* d_out,
                                         int64_t ldo, const float* lse, void* dq, void* dkv, void* workspace, size_t workspace_bytes,
                                         int64_t B, int64_t heads, int64_t head_dim, int64_t N, int64_t Nk, float scale, void* stream) {
    int rc = attn_check("mit_attention_bwd", q, kv, B, heads, head_dim, N, Nk, ldq, ldkv, ldo);
    if (rc) return rc;
    DIGA_REQUIRE(out && d_out && lse && dq && dkv && workspace, DIGA_EINVAL, "mit_attention_bwd: null pointer");
    DIGA_REQUIRE(ldkv == 2 * heads * head_dim, DIGA_EINVAL, "mit_attention_bwd: dkv is written densely, ldkv must be 2*heads*%lld",
                 (long long)head_dim);
    DIGA_REQUIRE(aligned16(out) && aligned16(d_out) && aligned16(dq) && aligned16(dkv) && aligned16(workspace), DIGA_EALIGN,
                 "mit_attention_bwd: alignment");
    const DkvPlan p = dkv_plan(B, heads, head_dim, N, Nk);
    DIGA_REQUIRE(workspace_bytes >= p.slab_bytes + (size_t)B * heads * N * sizeof(float), DIGA_EWORKSPACE, "mit_attention_bwd: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    AttnArgs a{};
    a.Q = static_cast<const _Float16*>(q); a.K = static_cast<const _Float16*>(kv); a.V = a.K + heads * head_dim;
    a.ldq = ldq; a.ldkv = ldkv; a.O = const_cast<_Float16*>(static_cast<const _Float16*>(out)); a.ldo = ldo;
    a.lse = const_cast<float*>(lse); a.dO = static_cast<const _Float16*>(d_out); a.dQ = static_cast<_Float16*>(dq);
    a.slab = static_cast<float*>(workspace);
    a.delta = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + p.slab_bytes);
    a.B = (int)B; a.heads = (int)heads; a.N = (int)N; a.Nk = (int)Nk;
    a.q_blocks = (int)ceil_div(N, 256);
    a.k_blocks = p.k_blocks; a.splits = p.splits; a.qblocks_per_split = p.qblocks_per_split;
    a.scale = scale; a.scale_log2e = scale * 1.4426950408889634f;
    ProfScope prof(DIGA_PROF_MIT_ATTN_BWD, st, 14.0 * (double)B * heads * (double)N * (double)Nk * (double)head_dim);
    if (head_dim == 64) launch_bwd<64>(a, static_cast<_Float16*>(dkv), st);
    else launch_bwd<32>(a, static_cast<_Float16*>(dkv), st);
    return launch_status("mit_attention_bwd");
}

extern "C" int diga_mit_attention_bwd(const void* q, int64_t ldq, const void* kv, int64_t ldkv, const void* out, const void* d_out,
                                      int64_t ldo, const float* lse, void* dq, void* dkv, void* workspace, size_t workspace_bytes,
                                      int64_t B, int64_t heads, int64_t N, int64_t Nk, float scale, void* stream) {
    return diga_mit_attention_hd_bwd(q, ldq, kv, ldkv, out, d_out, ldo, lse, dq, dkv, workspace, workspace_bytes, B, heads, 64, N, Nk, scale,
                                     stream);
}
