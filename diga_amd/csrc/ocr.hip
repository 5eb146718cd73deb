// Object-contextual representations: the two attention-shaped operations of the OCR head.
// Reference: semi-supervised_segmentation/model/networks/ocrnet_module.py:24-44 (ORegionModule: softmax over the pixels of every class
// map, then [K x P] by [P x C]), :77-95 and :231 (PixelRegionRelationModule + the value product: K-way softmax per pixel against K keys,
// then [P x K] by [K x Dv]).  K <= 32 classes against 10^4 .. 10^5 pixels: stock torch forms three [N, P, K] intermediates and runs two
// skinny batched GEMMs; both operations are ~10 FLOP per byte, i.e. bandwidth-bound.
//
// Two kernel shapes cover the four entry points (exact fp32 on the VALU -- at 10 FLOP per byte the fp32 MFMA has nothing to win, and K
// padded to 32 columns would waste 40 % of it at K = 19):
//   weighted pixel sums  out[k, :] = sum_p w[p, k] x[p, :]   (region gather; d_key and d_val of the attention backward)
//       block = 256 pixels of one image; the K weights of its pixels sit in LDS, a thread owns four channels and KT accumulator
//       quads, the pixel rows of the block are split over 256 / (C / 4) thread groups.  Per-block partials go to the workspace and a
//       second kernel adds them in block order (no float atomics: bit-reproducible).  The region gather takes its softmax ONLINE:
//       a block subtracts the maximum of its own pixels, the reduce kernel rescales by exp(m_block - m).
//   per-pixel K-vectors   g[k] = <x[p], M[k]>,  y[p, :] = sum_k c[k] M'[k, :]   (region backward, attention forward and backward)
//       a wave per pixel: the K x C matrices of the image sit in LDS for the whole block, a lane owns C / 64 channels, the K dot
//       products are finished by recursive halving over the wave (K + 2 shuffles, a lane pair per class: the softmax runs across
//       the lanes), the K coefficients are then read back into every lane with v_readlane.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace diga {

constexpr int kOcrKMax = 32;
constexpr int kOcrCMax = 1024;
constexpr int kOcrChunk = 256;        // pixels per block of the weighted-sum kernels (= one partial)
constexpr int kOcrPixBlock = 128;     // pixels per block of the wave-per-pixel kernels
constexpr size_t kOcrLdsMax = 160 * 1024;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void fma4(float4& a, float w, const float4& v) {
    a.x = fmaf(w, v.x, a.x);
    a.y = fmaf(w, v.y, a.y);
    a.z = fmaf(w, v.z, a.z);
    a.w = fmaf(w, v.w, a.w);
}

struct d4 {
    double x, y, z, w;
};
__device__ __forceinline__ void fma4(d4& a, float w, const float4& v) {
    const double wd = (double)w;
    a.x = fma(wd, (double)v.x, a.x);
    a.y = fma(wd, (double)v.y, a.y);
    a.z = fma(wd, (double)v.z, a.z);
    a.w = fma(wd, (double)v.w, a.w);
}

// ------------------------------------------------------------------------------------------ weighted pixel sums
// The region gather (SOFTMAX) accumulates, stores its partials and reduces in float64 and hands the backward pass its result as a
// pair (region = the nearest fp32, stat's low-order part = what that rounding dropped): the one-pass backward subtracts
// dot[k] = <d_region[k], region[k]> from every pixel's g, and sum_p w (g - dot) -- the gradient a bias in front of s gets -- vanishes
// only as far as `region` IS sum_p e x / sum_p e.  With an fp32 sum its own rounding times |d_region| stays in that gradient (4e-5 where a
// softmax backward that never forms `region` leaves 1e-5).  (Approximately so even now: the backward's weight is the rounded fp32
// product expf(s - m) * rl, the forward's exp(s - m_block) * exp(m_block - m) * rl unrounded -- a random 1e-7 per pixel, against the
// systematic 1e-7 of a whole fp32 sum.)  The plain sums (d_key, d_val) stay fp32.
// SOFTMAX: `s` holds logits; the weights are exp(s - m_block) and (m_block, sum of weights) go to `ml` [N][nblk][K][2].
// else   : the weights are alpha * s.
// part [N][nblk][K][C].  Grid (nblk, N, channel tiles of TX quads); TX = 1 << tx_log2 <= 128 threads across the channels.
template <int KT, bool SOFTMAX>
__global__ __launch_bounds__(256) void ocr_wsum_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ s, int64_t ld_s,
                                                       float alpha, float* __restrict__ part, float* __restrict__ ml, int64_t P, int K,
                                                       int C, int tx_log2) {
    __shared__ __align__(16) float wsm[kOcrChunk * KT];       // [pixel][KT] weights
    using acc_t = typename std::conditional<SOFTMAX, d4, float4>::type;
    __shared__ acc_t red[256];
    __shared__ float tmpm[8 * KT];
    __shared__ double tmpl[8 * KT];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int64_t nblk = gridDim.x, blk = blockIdx.x;
    const int64_t p0 = blk * kOcrChunk;
    const int np = (int)((P - p0) < kOcrChunk ? (P - p0) : kOcrChunk);
    const float* sp = s + ((int64_t)n * P + p0) * ld_s;
    for (int i = tid; i < kOcrChunk * KT; i += 256) {
        const int p = i / KT, k = i - p * KT;
        float v = 0.f;
        if (p < np && k < K) v = sp[(int64_t)p * ld_s + k] * (SOFTMAX ? 1.f : alpha);
        wsm[i] = v;
    }
    __syncthreads();
    if (SOFTMAX) {
        // eight threads per class, each a fixed stride-8 subset of the block's pixels; combined in subset order
        const int j = tid / KT, k = tid - j * KT;
        if (tid < 8 * KT) {
            float m = -INFINITY;
            for (int p = j; p < np; p += 8) m = fmaxf(m, wsm[p * KT + k]);
            tmpm[j * KT + k] = m;
        }
        __syncthreads();
        if (tid < 8 * KT) {
            float m = tmpm[k];
#pragma unroll
            for (int jj = 1; jj < 8; ++jj) m = fmaxf(m, tmpm[jj * KT + k]);
            double l = 0.0;
            for (int p = j; p < np; p += 8) {
                const float e = (k < K) ? expf(wsm[p * KT + k] - m) : 0.f;
                wsm[p * KT + k] = e;
                l += (double)e;
            }
            tmpl[j * KT + k] = l;
        }
        __syncthreads();
        if (tid < K && blockIdx.z == 0) {
            float m = tmpm[tid];
            double l = tmpl[tid];
#pragma unroll
            for (int jj = 1; jj < 8; ++jj) {
                m = fmaxf(m, tmpm[jj * KT + tid]);
                l += tmpl[jj * KT + tid];
            }
            double* o = reinterpret_cast<double*>(ml) + (((int64_t)n * nblk + blk) * K + tid) * 2;
            o[0] = (double)m;
            o[1] = l;
        }
    }
    const int TX = 1 << tx_log2, TY = 256 >> tx_log2;
    const int tx = tid & (TX - 1), ty = tid >> tx_log2;
    const int cq = C >> 2;
    const int q = blockIdx.z * TX + tx;
    const bool active = q < cq;
    acc_t acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = acc_t{0, 0, 0, 0};
    const float* xp = x + ((int64_t)n * P + p0) * ld_x + 4 * (active ? q : 0);
    constexpr int U = 4;                  // pixel rows in flight per thread
    for (int pb = ty; pb < np; pb += U * TY) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = pb + u * TY;
            v[u] = (active && p < np) ? ld4(xp + (int64_t)p * ld_x) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = pb + u * TY;
            if (p < np) {                 // (p <= 255: rows past np hold zero weights, but are never read anyway)
                const float* w = wsm + p * KT;
#pragma unroll
                for (int k4 = 0; k4 < KT; k4 += 4) {
                    const float4 w4 = ld4(w + k4);
                    fma4(acc[k4 + 0], w4.x, v[u]);
                    fma4(acc[k4 + 1], w4.y, v[u]);
                    fma4(acc[k4 + 2], w4.z, v[u]);
                    fma4(acc[k4 + 3], w4.w, v[u]);
                }
            }
        }
    }
    // the TY row groups of a channel quad, added in group order
    const int64_t po = (((int64_t)n * nblk + blk) * K) * C + 4 * (active ? q : 0);       // (in floats, or in doubles under SOFTMAX)
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (k < K) {
            __syncthreads();
            red[tid] = acc[k];
            __syncthreads();
            if (ty == 0 && active) {
                acc_t t = red[tx];
                for (int g = 1; g < TY; ++g) {
                    const acc_t r = red[g * TX + tx];
                    t.x += r.x;
                    t.y += r.y;
                    t.z += r.z;
                    t.w += r.w;
                }
                if constexpr (SOFTMAX) *reinterpret_cast<d4*>(reinterpret_cast<double*>(part) + po + (int64_t)k * C) = t;
                else st4(part + po + (int64_t)k * C, t);
            }
        }
    }
}

// out [N][K][C] = sum over the nblk partials, in block order.  SOFTMAX: partial b counts exp(m_b - m) times and the total is scaled by
// 1 / (rescaled sum of weights).
template <bool SOFTMAX>
__global__ __launch_bounds__(256) void ocr_wsum_reduce_kernel(const float* __restrict__ part, const float* __restrict__ ml,
                                                              float* __restrict__ out, float* __restrict__ stat, int64_t nblk, int K,
                                                              int C) {
    const int n = blockIdx.y;
    const int N = gridDim.y;
    const int cq = C >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * cq) return;
    const int k = idx / cq, q = idx - k * cq;
    const int64_t o = ((int64_t)n * K + k) * C + 4 * q;
    if constexpr (SOFTMAX) {
        // float64 throughout; stat = [N][K][C] low-order part of the result, then [N][K][2] (maximum, 1 / sum)
        const double* pp = reinterpret_cast<const double*>(part) + ((int64_t)n * nblk * K + k) * C + 4 * q;
        const double* mp = reinterpret_cast<const double*>(ml) + ((int64_t)n * nblk * K + k) * 2;
        double m = -INFINITY;
        for (int64_t b = 0; b < nblk; ++b) m = fmax(m, mp[b * K * 2]);
        double l = 0.0, tx = 0.0, ty = 0.0, tz = 0.0, tw = 0.0;
        for (int64_t b = 0; b < nblk; ++b) {
            const double f = (double)expf((float)(mp[b * K * 2] - m));           // (the maxima are fp32 values: the difference is exact)
            l = fma(f, mp[b * K * 2 + 1], l);
            const d4 r = *reinterpret_cast<const d4*>(pp + b * K * C);
            tx = fma(f, r.x, tx);
            ty = fma(f, r.y, ty);
            tz = fma(f, r.z, tz);
            tw = fma(f, r.w, tw);
        }
        // normalised by the float64 1 / l, NOT by the fp32 rl the backward weighs with: its weights e * rl sum to W = l * rl = 1 + d,
        // |d| <= 6e-8, so sum_p w g = W <d_region, sum e x / l> and sum_p w (g - dot) = W dot_here - dot W = 0 only with THIS dot
        // (with the sum scaled by rl the class with the largest dot kept d * dot: 2.2e-6 of the bias gradient's scale, measured)
        const double inv = 1.0 / l;
        const float rl = (float)inv;
        tx *= inv;
        ty *= inv;
        tz *= inv;
        tw *= inv;
        const float4 hi = make_float4((float)tx, (float)ty, (float)tz, (float)tw);
        st4(out + o, hi);
        st4(stat + o, make_float4((float)(tx - (double)hi.x), (float)(ty - (double)hi.y), (float)(tz - (double)hi.z), (float)(tw - (double)hi.w)));
        if (q == 0) {
            float* st2 = stat + (int64_t)N * K * C + ((int64_t)n * K + k) * 2;
            st2[0] = (float)m;
            st2[1] = rl;
        }
    } else {
        const float* pp = part + ((int64_t)n * nblk * K + k) * C + 4 * q;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t b = 0; b < nblk; ++b) {
            const float4 r = ld4(pp + b * K * C);
            t.x += r.x;
            t.y += r.y;
            t.z += r.z;
            t.w += r.w;
        }
        st4(out + o, t);
    }
}

// ------------------------------------------------------------------------------------------ wave-per-pixel pieces
// A lane owns the channel quads lane, lane + 64, ... (NQ of them; quads past cq read as zero and are never written).
template <int NQ>
__device__ __forceinline__ void load_row(float4 (&v)[NQ], const float* __restrict__ row, int cq, int lane) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = lane + 64 * i;
        v[i] = q < cq ? ld4(row + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// g[k] = this lane's share of <row, mat[k]> for every k < KT.  mat: LDS [KT][ldm], rows past K hold zeros.
template <int KT, int NQ>
__device__ __forceinline__ void dot_rows(float (&g)[KT], const float4 (&v)[NQ], const float* mat, int ldm, int cq, int lane) {
#pragma unroll
    for (int k = 0; k < KT; ++k) g[k] = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = lane + 64 * i;
        if (q < cq) {
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float4 m = ld4(mat + k * ldm + 4 * q);
                g[k] = fmaf(v[i].w, m.w, fmaf(v[i].z, m.z, fmaf(v[i].y, m.y, fmaf(v[i].x, m.x, g[k]))));
            }
        }
    }
}

// Sum of KT per-lane values over the wave by recursive halving: at the step of lane bit M a lane keeps one half of its live values
// (the upper half when its bit is set), hands the other half to its partner and adds what it gets -- KT + 2 shuffles in all instead
// of 6 KT for KT butterflies.  Afterwards lane l holds the complete sum of value ocr_lane_k(l) (lanes l and l ^ 1 the same one);
// a lane whose halves ran out holds padding.
template <int KT, int N, int M, typename T>
__device__ __forceinline__ void rs_step(T (&v)[KT], int lane) {
    if constexpr (M >= 2) {
        constexpr int H = (N + 1) / 2;
        const bool up = (lane & M) != 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const T lo = v[i], hi = (i + H < N) ? v[i + H] : T(0);
            const T send = up ? lo : hi, keep = up ? hi : lo;
            v[i] = keep + __shfl_xor(send, M, 64);
        }
        rs_step<KT, H, M / 2>(v, lane);
    }
}
template <int KT, typename T>
__device__ __forceinline__ T reduce_scatter(T (&v)[KT], int lane) {
    rs_step<KT, KT, 32>(v, lane);
    return v[0] + __shfl_xor(v[0], 1, 64);
}
// the value index lane `lane` ends up with, or -1 (padding, or an index >= K)
template <int KT>
__device__ __forceinline__ int ocr_lane_k(int lane, int K) {
    int base = 0, cnt = K, ns = KT;
#pragma unroll
    for (int m = 32; m >= 2; m >>= 1) {
        const int h = (ns + 1) / 2;
        if (lane & m) {
            base += h;
            cnt -= h;
        } else {
            cnt = cnt < h ? cnt : h;
        }
        ns = h;
    }
    return cnt >= 1 ? base : -1;
}
// ... and the (even) lane that holds value k
template <int KT>
__host__ __device__ constexpr int ocr_k_lane(int k) {
    int lane = 0, ns = KT;
    for (int m = 32; m >= 2; m >>= 1) {
        const int h = (ns + 1) / 2;
        if (k >= h) {
            lane |= m;
            k -= h;
        }
        ns = h;
    }
    return lane;
}
// every lane's value -> all KT of them in every lane (v_readlane of a constant lane)
template <int KT>
__device__ __forceinline__ void gather_k(float (&c)[KT], float mine) {
#pragma unroll
    for (int k = 0; k < KT; ++k) c[k] = __shfl(mine, ocr_k_lane<KT>(k), 64);
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// row[:] = sum_k c[k] mat[k, :] * post
template <int KT, int NQ>
__device__ __forceinline__ void combine_rows(float* __restrict__ row, const float (&c)[KT], const float* mat, int ldm, int cq, int lane,
                                             float post) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = lane + 64 * i;
        if (q < cq) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < KT; ++k) fma4(o, c[k], ld4(mat + k * ldm + 4 * q));
            o.x *= post;
            o.y *= post;
            o.z *= post;
            o.w *= post;
            st4(row + 4 * q, o);
        }
    }
}

// mat [K][C] dense in global memory -> LDS [KT][C], rows past K zeroed
template <int KT>
__device__ __forceinline__ void stage_rows(float* dst, const float* __restrict__ src, int K, int C) {
    const int cq = C >> 2;
    for (int i = threadIdx.x; i < KT * cq; i += 256) {
        const int k = i / cq;
        st4(dst + 4 * i, k < K ? ld4(src + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// ------------------------------------------------------------------------------------------ region backward
template <int KT, int NQ>
__global__ __launch_bounds__(256) void ocr_region_bwd_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ s,
                                                             int64_t ld_s, const float* __restrict__ stat, const float* __restrict__ region,
                                                             const float* __restrict__ d_region, float* __restrict__ dx, int64_t ld_dx,
                                                             float* __restrict__ ds, int64_t ld_ds, int64_t P, int K, int C) {
    extern __shared__ __align__(16) float smem[];
    float* dR = smem;                     // [KT][C]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int cq = C >> 2;
    stage_rows<KT>(dR, d_region + (int64_t)n * K * C, K, C);
    __syncthreads();
    // dot[k] = <region[k] + its low-order part, d_region[k]> in float64 (every wave for its own lanes, the same in every block), and
    // g - dot is taken in float64 too: see the note at the weighted pixel sums
    const int myk = ocr_lane_k<KT>(lane, K);
    const bool lk = myk >= 0 && (lane & 1) == 0;          // the even lane of a pair owns the class
    double dotk;
    {
        double t[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            t[k] = 0.0;
            if (k < K) {
                float4 r[NQ], rlo[NQ];
                load_row<NQ>(r, region + ((int64_t)n * K + k) * C, cq, lane);
                load_row<NQ>(rlo, stat + ((int64_t)n * K + k) * C, cq, lane);
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
                    const int q = lane + 64 * i;
                    if (q < cq) {
                        const float4 m = ld4(dR + k * C + 4 * q);
                        t[k] = fma((double)r[i].x + (double)rlo[i].x, (double)m.x, t[k]);
                        t[k] = fma((double)r[i].y + (double)rlo[i].y, (double)m.y, t[k]);
                        t[k] = fma((double)r[i].z + (double)rlo[i].z, (double)m.z, t[k]);
                        t[k] = fma((double)r[i].w + (double)rlo[i].w, (double)m.w, t[k]);
                    }
                }
            }
        }
        dotk = reduce_scatter<KT>(t, lane);
    }
    const float* st2 = stat + (int64_t)gridDim.y * K * C;          // [N][K][2] behind the low-order parts
    const float mk = lk ? st2[((int64_t)n * K + myk) * 2] : 0.f, rl = lk ? st2[((int64_t)n * K + myk) * 2 + 1] : 0.f;
    const int64_t p0 = (int64_t)blockIdx.x * kOcrPixBlock;
    const int64_t pend = (p0 + kOcrPixBlock < P) ? p0 + kOcrPixBlock : P;
    const int64_t base = (int64_t)n * P;
    float4 v[NQ], vn[NQ];
    int64_t p = p0 + wv;
    if (p < pend) load_row<NQ>(v, x + (base + p) * ld_x, cq, lane);
    for (; p < pend; p += 4) {
        const float sl = lk ? s[(base + p) * ld_s + myk] : 0.f;
        if (p + 4 < pend) load_row<NQ>(vn, x + (base + p + 4) * ld_x, cq, lane);
        float g[KT];
        dot_rows<KT, NQ>(g, v, dR, C, cq, lane);
        const float gk = reduce_scatter<KT>(g, lane);
        const float wl = lk ? expf(sl - mk) * rl : 0.f;
        if (lk) ds[(base + p) * ld_ds + myk] = wl * (float)((double)gk - dotk);
        float w[KT];
        gather_k<KT>(w, wl);
        combine_rows<KT, NQ>(dx + (base + p) * ld_dx, w, dR, C, cq, lane, 1.f);
#pragma unroll
        for (int i = 0; i < NQ; ++i) v[i] = vn[i];
    }
}

// ------------------------------------------------------------------------------------------ object attention
// LDS: key [KT][D], val [KT][Dv] of the block's image.
template <int KT, int NQ>
__global__ __launch_bounds__(256) void ocr_attend_fwd_kernel(const float* __restrict__ qm, int64_t ld_q, const float* __restrict__ key,
                                                             const float* __restrict__ val, float* __restrict__ out, int64_t ld_out,
                                                             float* __restrict__ attn, int64_t P, int K, int D, int Dv, float scale) {
    extern __shared__ __align__(16) float smem[];
    float* kS = smem;
    float* vS = smem + KT * D;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.y;
    stage_rows<KT>(kS, key + (int64_t)n * K * D, K, D);
    stage_rows<KT>(vS, val + (int64_t)n * K * Dv, K, Dv);
    __syncthreads();
    const int dq_ = D >> 2, dvq = Dv >> 2;
    const int64_t p0 = (int64_t)blockIdx.x * kOcrPixBlock;
    const int64_t pend = (p0 + kOcrPixBlock < P) ? p0 + kOcrPixBlock : P;
    const int64_t base = (int64_t)n * P;
    const int myk = ocr_lane_k<KT>(lane, K);
    const bool lk = myk >= 0 && (lane & 1) == 0;          // the even lane of a pair owns the class
    // two pixels per wave and round: a key / value quad read from LDS serves both (the LDS reads, not HBM, bounded the one-pixel form)
    float4 v0[NQ], v1[NQ], n0[NQ], n1[NQ];
    int64_t p = p0 + 2 * wv;
    if (p < pend) {
        load_row<NQ>(v0, qm + (base + p) * ld_q, dq_, lane);
        load_row<NQ>(v1, qm + (base + (p + 1 < pend ? p + 1 : p)) * ld_q, dq_, lane);
    }
    for (; p < pend; p += 8) {
        const bool two = p + 1 < pend;
        if (p + 8 < pend) {
            load_row<NQ>(n0, qm + (base + p + 8) * ld_q, dq_, lane);
            load_row<NQ>(n1, qm + (base + (p + 9 < pend ? p + 9 : p + 8)) * ld_q, dq_, lane);
        }
        float a0[KT], a1[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) a0[k] = a1[k] = 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = lane + 64 * i;
            if (q < dq_) {
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const float4 m = ld4(kS + k * D + 4 * q);
                    a0[k] = fmaf(v0[i].w, m.w, fmaf(v0[i].z, m.z, fmaf(v0[i].y, m.y, fmaf(v0[i].x, m.x, a0[k]))));
                    a1[k] = fmaf(v1[i].w, m.w, fmaf(v1[i].z, m.z, fmaf(v1[i].y, m.y, fmaf(v1[i].x, m.x, a1[k]))));
                }
            }
        }
        const float r0 = reduce_scatter<KT>(a0, lane), r1 = reduce_scatter<KT>(a1, lane);      // (every lane runs the shuffles)
        const float l0 = lk ? scale * r0 : -INFINITY, l1 = lk ? scale * r1 : -INFINITY;
        const float m0 = wave_max(l0), m1 = wave_max(l1);
        const float e0 = lk ? expf(l0 - m0) : 0.f, e1 = lk ? expf(l1 - m1) : 0.f;
        const float al0 = e0 * (1.f / wave_sum(e0)), al1 = e1 * (1.f / wave_sum(e1));
        if (attn != nullptr && lk) {
            attn[(base + p) * K + myk] = al0;
            if (two) attn[(base + p + 1) * K + myk] = al1;
        }
        gather_k<KT>(a0, al0);
        gather_k<KT>(a1, al1);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = lane + 64 * i;
            if (q < dvq) {
                float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = o0;
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const float4 m = ld4(vS + k * Dv + 4 * q);
                    fma4(o0, a0[k], m);
                    fma4(o1, a1[k], m);
                }
                st4(out + (base + p) * ld_out + 4 * q, o0);
                if (two) st4(out + (base + p + 1) * ld_out + 4 * q, o1);
            }
        }
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            v0[i] = n0[i];
            v1[i] = n1[i];
        }
    }
}

// dl [N][P][K] (workspace) and dq; d_key / d_val are weighted pixel sums of q under scale * dl and of d_out under attn.
template <int KT, int NQ>
__global__ __launch_bounds__(256) void ocr_attend_bwd_kernel(const float* __restrict__ key, const float* __restrict__ val,
                                                             const float* __restrict__ attn, const float* __restrict__ d_out, int64_t ld_do,
                                                             float* __restrict__ dq, int64_t ld_dq, float* __restrict__ dl, int64_t P, int K,
                                                             int D, int Dv, float scale) {
    extern __shared__ __align__(16) float smem[];
    float* kS = smem;
    float* vS = smem + KT * D;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.y;
    stage_rows<KT>(kS, key + (int64_t)n * K * D, K, D);
    stage_rows<KT>(vS, val + (int64_t)n * K * Dv, K, Dv);
    __syncthreads();
    const int dq_ = D >> 2, dvq = Dv >> 2;
    const int64_t p0 = (int64_t)blockIdx.x * kOcrPixBlock;
    const int64_t pend = (p0 + kOcrPixBlock < P) ? p0 + kOcrPixBlock : P;
    const int64_t base = (int64_t)n * P;
    const int myk = ocr_lane_k<KT>(lane, K);
    const bool lk = myk >= 0 && (lane & 1) == 0;          // the even lane of a pair owns the class
    float4 v[NQ], vn[NQ];
    int64_t p = p0 + wv;
    if (p < pend) load_row<NQ>(v, d_out + (base + p) * ld_do, dvq, lane);
    for (; p < pend; p += 4) {
        const float al = lk ? attn[(base + p) * K + myk] : 0.f;
        if (p + 4 < pend) load_row<NQ>(vn, d_out + (base + p + 4) * ld_do, dvq, lane);
        float dA[KT];
        dot_rows<KT, NQ>(dA, v, vS, Dv, dvq, lane);
        const float dAk = reduce_scatter<KT>(dA, lane);
        const float sum = wave_sum(lk ? al * dAk : 0.f);
        const float dlk = lk ? al * (dAk - sum) : 0.f;
        if (lk) dl[(base + p) * K + myk] = dlk;
        gather_k<KT>(dA, dlk);
        combine_rows<KT, NQ>(dq + (base + p) * ld_dq, dA, kS, D, dq_, lane, scale);
#pragma unroll
        for (int i = 0; i < NQ; ++i) v[i] = vn[i];
    }
}

// ------------------------------------------------------------------------------------------ host side
static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
static inline int64_t ocr_nblk(int64_t P) { return ceil_div(P, kOcrChunk); }
static inline bool ocr_shape_ok(int64_t N, int64_t P, int64_t K, int64_t C) {
    return N >= 1 && N <= 65535 && P >= 1 && K >= 1 && K <= kOcrKMax && C >= 4 && C <= kOcrCMax && C % 4 == 0;
}
// (float64 partials and (maximum, sum) pairs of the region gather: two floats each)
static inline size_t ocr_part_floats(int64_t N, int64_t P, int64_t K, int64_t C) { return (size_t)N * ocr_nblk(P) * K * (2 * C + 4); }

// KT: the class count rounded up to a multiple of 4 (16, 19 -> 20, 22 -> 24 are the sizes of the path), as a template argument
#define DIGA_OCR_KT(K_, CALL_)                   \
    do {                                         \
        if (K_ <= 16) { CALL_(16); }             \
        else if (K_ <= 20) { CALL_(20); }        \
        else if (K_ <= 24) { CALL_(24); }        \
        else { CALL_(32); }                      \
    } while (0)
#define DIGA_OCR_KT_NQ(K_, NQ_, CALL_)                                    \
    do {                                                                 \
        if (NQ_ == 1) { DIGA_OCR_KT(K_, CALL_##_1); }                    \
        else if (NQ_ == 2) { DIGA_OCR_KT(K_, CALL_##_2); }               \
        else { DIGA_OCR_KT(K_, CALL_##_4); }                             \
    } while (0)

static inline int ocr_kt(int64_t K) { return K <= 16 ? 16 : K <= 20 ? 20 : K <= 24 ? 24 : 32; }
static inline int ocr_nq(int64_t C) { return C <= 256 ? 1 : C <= 512 ? 2 : 4; }

// out [N][K][C] = sum_p w[p, k] x[p, :]: the two launches.  part / ml inside the workspace.
template <bool SOFTMAX>
static void ocr_wsum_launch(const float* x, int64_t ld_x, const float* s, int64_t ld_s, float alpha, float* out, float* stat, float* part,
                            int64_t N, int64_t P, int64_t K, int64_t C, hipStream_t st) {
    const int64_t nblk = ocr_nblk(P);
    float* ml = part + (size_t)N * nblk * K * C * (SOFTMAX ? 2 : 1);
    const int cq = (int)(C / 4);
    int tx_log2 = 0;
    while ((1 << tx_log2) < cq && tx_log2 < 7) ++tx_log2;
    const dim3 grid((unsigned)nblk, (unsigned)N, (unsigned)ceil_div(cq, 1 << tx_log2));
#define DIGA_OCR_WSUM(KT_)                                                                                                             \
    hipLaunchKernelGGL((ocr_wsum_kernel<KT_, SOFTMAX>), grid, dim3(256), 0, st, x, ld_x, s, ld_s, alpha, part, ml, P, (int)K, (int)C, \
                       tx_log2)
    DIGA_OCR_KT(K, DIGA_OCR_WSUM);
#undef DIGA_OCR_WSUM
    hipLaunchKernelGGL((ocr_wsum_reduce_kernel<SOFTMAX>), dim3((unsigned)ceil_div(K * cq, 256), (unsigned)N), dim3(256), 0, st, part, ml,
                       out, stat, nblk, (int)K, (int)C);
}

}  // namespace diga

using namespace diga;

extern "C" size_t diga_ocr_workspace_bytes(int64_t N, int64_t P, int64_t K, int64_t C) {
    if (!ocr_shape_ok(N, P, K, C)) return 0;
    // [N][P][K] (dl of the attention backward) + the partials [N][nblk][K][C] with their (maximum, sum) pairs
    return ((size_t)N * P * K + 4 + ocr_part_floats(N, P, K, C)) * sizeof(float);
}

#define DIGA_OCR_SHAPE(name, N, P, K)                                                                                              \
    DIGA_REQUIRE(K >= 1 && K <= kOcrKMax, DIGA_EINVAL, name ": K = %lld outside 1 .. 32", (long long)K);                          \
    DIGA_REQUIRE(N >= 1 && N <= 65535 && P >= 1, DIGA_EINVAL, name ": bad shape N = %lld (1 .. 65535), P = %lld", (long long)N, \
                 (long long)P)
#define DIGA_OCR_CHANNELS(name, what, C)                                                                                               \
    DIGA_REQUIRE(C >= 4 && C % 4 == 0, DIGA_EINVAL, name ": channel count " what " = %lld is not a positive multiple of 4", (long long)C); \
    DIGA_REQUIRE(C <= kOcrCMax, DIGA_EINVAL, name ": channel count " what " = %lld above 1024", (long long)C)
#define DIGA_OCR_PITCH(name, what, ld, C)                                                                                   \
    DIGA_REQUIRE(ld >= C, DIGA_EINVAL, name ": pitch " what " = %lld smaller than the row of %lld", (long long)ld, (long long)C)
#define DIGA_OCR_PITCH4(name, what, ld, C) \
    DIGA_OCR_PITCH(name, what, ld, C);     \
    DIGA_REQUIRE(ld % 4 == 0, DIGA_EINVAL, name ": pitch " what " = %lld is not a multiple of 4", (long long)ld)

extern "C" int diga_ocr_region_fwd(const float* x, int64_t ld_x, const float* s, int64_t ld_s, float* region, float* stat, int64_t N,
                                   int64_t P, int64_t K, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    DIGA_REQUIRE(x && s && region && stat && workspace, DIGA_EINVAL, "ocr_region_fwd: null pointer");
    DIGA_REQUIRE(aligned16(x) && aligned16(region) && aligned16(workspace) && aligned4(s) && aligned16(stat), DIGA_EINVAL,
                 "ocr_region_fwd: misaligned pointer (x, region, stat, workspace: 16 bytes; s: 4)");
    DIGA_OCR_SHAPE("ocr_region_fwd", N, P, K);
    DIGA_OCR_CHANNELS("ocr_region_fwd", "C", C);
    DIGA_OCR_PITCH4("ocr_region_fwd", "ld_x", ld_x, C);
    DIGA_OCR_PITCH("ocr_region_fwd", "ld_s", ld_s, K);
    DIGA_REQUIRE(workspace_bytes >= diga_ocr_workspace_bytes(N, P, K, C), DIGA_EINVAL, "ocr_region_fwd: workspace too small (%zu < %zu bytes)",
                 workspace_bytes, diga_ocr_workspace_bytes(N, P, K, C));
    float* part = (float*)workspace + (((size_t)N * P * K + 3) & ~(size_t)3);
    ocr_wsum_launch<true>(x, ld_x, s, ld_s, 1.f, region, stat, part, N, P, K, C, (hipStream_t)stream);
    return launch_status("diga_ocr_region_fwd");
}

extern "C" int diga_ocr_region_bwd(const float* x, int64_t ld_x, const float* s, int64_t ld_s, const float* stat, const float* region,
                                   const float* d_region, float* dx, int64_t ld_dx, float* ds, int64_t ld_ds, int64_t N, int64_t P,
                                   int64_t K, int64_t C, void* stream) {
    DIGA_REQUIRE(x && s && stat && region && d_region && dx && ds, DIGA_EINVAL, "ocr_region_bwd: null pointer");
    DIGA_REQUIRE(aligned16(x) && aligned16(region) && aligned16(d_region) && aligned16(dx) && aligned4(s) && aligned16(stat) && aligned4(ds),
                 DIGA_EINVAL, "ocr_region_bwd: misaligned pointer (x, region, d_region, dx, stat: 16 bytes; s, ds: 4)");
    DIGA_OCR_SHAPE("ocr_region_bwd", N, P, K);
    DIGA_OCR_CHANNELS("ocr_region_bwd", "C", C);
    DIGA_OCR_PITCH4("ocr_region_bwd", "ld_x", ld_x, C);
    DIGA_OCR_PITCH4("ocr_region_bwd", "ld_dx", ld_dx, C);
    DIGA_OCR_PITCH("ocr_region_bwd", "ld_s", ld_s, K);
    DIGA_OCR_PITCH("ocr_region_bwd", "ld_ds", ld_ds, K);
    hipStream_t st = (hipStream_t)stream;
    const int nq = ocr_nq(C);
    const size_t sh = (size_t)ocr_kt(K) * C * sizeof(float);                    // <= 32 * 1024 * 4 bytes
    const dim3 grid((unsigned)ceil_div(P, kOcrPixBlock), (unsigned)N);
#define DIGA_OCR_RB(KT_, NQ_)                                                                                                             \
    do {                                                                                                                                  \
        (void)hipFuncSetAttribute((const void*)ocr_region_bwd_kernel<KT_, NQ_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);     \
        hipLaunchKernelGGL((ocr_region_bwd_kernel<KT_, NQ_>), grid, dim3(256), sh, st, x, ld_x, s, ld_s, stat, region, d_region, dx, ld_dx, \
                           ds, ld_ds, P, (int)K, (int)C);                                                                                 \
    } while (0)
#define DIGA_OCR_RB_1(KT_) DIGA_OCR_RB(KT_, 1)
#define DIGA_OCR_RB_2(KT_) DIGA_OCR_RB(KT_, 2)
#define DIGA_OCR_RB_4(KT_) DIGA_OCR_RB(KT_, 4)
    DIGA_OCR_KT_NQ(K, nq, DIGA_OCR_RB);
    return launch_status("diga_ocr_region_bwd");
}

#define DIGA_OCR_ATTEND_LDS(name, K, D, Dv)                                                                                     \
    DIGA_REQUIRE(((size_t)ocr_kt(K) * (D + Dv) + 64) * sizeof(float) <= kOcrLdsMax, DIGA_EINVAL,                                \
                 name ": keys and values of one image (K = %lld, D = %lld, Dv = %lld) do not fit the 160 KB of LDS", (long long)K, \
                 (long long)D, (long long)Dv)

extern "C" int diga_ocr_attend_fwd(const float* q, int64_t ld_q, const float* key, const float* val, float* out, int64_t ld_out, float* attn,
                                   int64_t N, int64_t P, int64_t K, int64_t D, int64_t Dv, float scale, void* stream) {
    DIGA_REQUIRE(q && key && val && out, DIGA_EINVAL, "ocr_attend_fwd: null pointer");
    DIGA_REQUIRE(aligned16(q) && aligned16(key) && aligned16(val) && aligned16(out) && aligned4(attn), DIGA_EINVAL,
                 "ocr_attend_fwd: misaligned pointer (q, key, val, out: 16 bytes; attn: 4)");
    DIGA_OCR_SHAPE("ocr_attend_fwd", N, P, K);
    DIGA_OCR_CHANNELS("ocr_attend_fwd", "D", D);
    DIGA_OCR_CHANNELS("ocr_attend_fwd", "Dv", Dv);
    DIGA_OCR_PITCH4("ocr_attend_fwd", "ld_q", ld_q, D);
    DIGA_OCR_PITCH4("ocr_attend_fwd", "ld_out", ld_out, Dv);
    DIGA_OCR_ATTEND_LDS("ocr_attend_fwd", K, D, Dv);
    hipStream_t st = (hipStream_t)stream;
    const int nq = ocr_nq(std::max(D, Dv));
    const size_t sh = (size_t)ocr_kt(K) * (D + Dv) * sizeof(float);
    const dim3 grid((unsigned)ceil_div(P, kOcrPixBlock), (unsigned)N);
#define DIGA_OCR_AF(KT_, NQ_)                                                                                                              \
    do {                                                                                                                                   \
        (void)hipFuncSetAttribute((const void*)ocr_attend_fwd_kernel<KT_, NQ_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);      \
        hipLaunchKernelGGL((ocr_attend_fwd_kernel<KT_, NQ_>), grid, dim3(256), sh, st, q, ld_q, key, val, out, ld_out, attn, P, (int)K,    \
                           (int)D, (int)Dv, scale);                                                                                        \
    } while (0)
#define DIGA_OCR_AF_1(KT_) DIGA_OCR_AF(KT_, 1)
#define DIGA_OCR_AF_2(KT_) DIGA_OCR_AF(KT_, 2)
#define DIGA_OCR_AF_4(KT_) DIGA_OCR_AF(KT_, 4)
    DIGA_OCR_KT_NQ(K, nq, DIGA_OCR_AF);
    return launch_status("diga_ocr_attend_fwd");
}

extern "C" int diga_ocr_attend_bwd(const float* q, int64_t ld_q, const float* key, const float* val, const float* attn, const float* d_out,
                                   int64_t ld_do, float* dq, int64_t ld_dq, float* d_key, float* d_val, int64_t N, int64_t P, int64_t K,
                                   int64_t D, int64_t Dv, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    DIGA_REQUIRE(q && key && val && attn && d_out && dq && d_key && d_val && workspace, DIGA_EINVAL, "ocr_attend_bwd: null pointer");
    DIGA_REQUIRE(aligned16(q) && aligned16(key) && aligned16(val) && aligned16(d_out) && aligned16(dq) && aligned16(d_key) &&
                     aligned16(d_val) && aligned16(workspace) && aligned4(attn),
                 DIGA_EINVAL, "ocr_attend_bwd: misaligned pointer (q, key, val, d_out, dq, d_key, d_val, workspace: 16 bytes; attn: 4)");
    DIGA_OCR_SHAPE("ocr_attend_bwd", N, P, K);
    DIGA_OCR_CHANNELS("ocr_attend_bwd", "D", D);
    DIGA_OCR_CHANNELS("ocr_attend_bwd", "Dv", Dv);
    DIGA_OCR_PITCH4("ocr_attend_bwd", "ld_q", ld_q, D);
    DIGA_OCR_PITCH4("ocr_attend_bwd", "ld_do", ld_do, Dv);
    DIGA_OCR_PITCH4("ocr_attend_bwd", "ld_dq", ld_dq, D);
    DIGA_OCR_ATTEND_LDS("ocr_attend_bwd", K, D, Dv);
    const int64_t cw = std::max(D, Dv);
    DIGA_REQUIRE(workspace_bytes >= diga_ocr_workspace_bytes(N, P, K, cw), DIGA_EINVAL, "ocr_attend_bwd: workspace too small (%zu < %zu bytes)",
                 workspace_bytes, diga_ocr_workspace_bytes(N, P, K, cw));
    hipStream_t st = (hipStream_t)stream;
    float* dl = (float*)workspace;
    float* part = dl + (((size_t)N * P * K + 3) & ~(size_t)3);
    const int nq = ocr_nq(cw);
    const size_t sh = (size_t)ocr_kt(K) * (D + Dv) * sizeof(float);
    const dim3 grid((unsigned)ceil_div(P, kOcrPixBlock), (unsigned)N);
#define DIGA_OCR_AB(KT_, NQ_)                                                                                                              \
    do {                                                                                                                                   \
        (void)hipFuncSetAttribute((const void*)ocr_attend_bwd_kernel<KT_, NQ_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);      \
        hipLaunchKernelGGL((ocr_attend_bwd_kernel<KT_, NQ_>), grid, dim3(256), sh, st, key, val, attn, d_out, ld_do, dq, ld_dq, dl, P,     \
                           (int)K, (int)D, (int)Dv, scale);                                                                                \
    } while (0)
#define DIGA_OCR_AB_1(KT_) DIGA_OCR_AB(KT_, 1)
#define DIGA_OCR_AB_2(KT_) DIGA_OCR_AB(KT_, 2)
#define DIGA_OCR_AB_4(KT_) DIGA_OCR_AB(KT_, 4)
    DIGA_OCR_KT_NQ(K, nq, DIGA_OCR_AB);
    // the two sums over pixels share the partials' slot: same stream, one after the other
    ocr_wsum_launch<false>(q, ld_q, dl, K, scale, d_key, nullptr, part, N, P, K, D, st);
    ocr_wsum_launch<false>(d_out, ld_do, attn, K, 1.f, d_val, nullptr, part, N, P, K, Dv, st);
    return launch_status("diga_ocr_attend_bwd");
}
