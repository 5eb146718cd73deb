// Backward-data of a stride-2 convolution with more than one tap, on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32).
//
//   dx[n, y, x, c] = sum_{r,s,k} dy[n, (y + pad_y - r)/2, (x + pad_x - s)/2, k] * w[k, r, s, c]      (exact quotients inside dy only)
//
// dx is split into its four phases (py, px) = (y & 1, x & 1).  With r0 = (py + pad_y) & 1 the rows of a phase see the taps
// r = r0 + 2t, t in [0, Rp), Rp = (R - r0 + 1) / 2, and row y = 2j + py reads dy row j + (py + pad_y - r0)/2 - t (columns alike):
// every phase is a stride-1 correlation of dy with a subset of the taps of the [Cin][R][S][Cout] transpose (diga_weight_transpose),
// addressed in place -- no gathered weight copy.  3x3 / pad 1 runs 1 + 2 + 2 + 4 = 9 tap-GEMMs over a quarter of the pixels each: the
// forward's multiplication count, a quarter of what the zero-inserted dy costs on the stride-1 backward-data kernel.
//
// One launch covers the four phases.  A block owns 128 pixels of ONE phase x 64 input channels, so all its rows share one tap list and
// the K loop is Rp * Sp * (Cout / 32) steps with no dead tap; the grid is the sum of the phases' tile counts (each rounded up to a multiple of 8, see
// the kernel) and a block finds its phase from the prefix table of block offsets in the kernel arguments.  Tiling, fragment mapping, the 36-float LDS rows, the register-staged double
// buffer, the clamped-address loader and the summation order (tap-major, channel-minor) are conv_fwd_kernel<1, 32>'s (conv.hip).
// A phase without taps (Rp == 0 or Sp == 0) and pixels no tap reaches run zero / all-masked K-steps and store zeros: the kernel writes
// every element of dx[.., :Cin].
#include "common.h"
#include "conv_call.h"

namespace diga {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4nt = __attribute__((ext_vector_type(4))) float;

constexpr int kBM = 128, kBN = 64, kBK = 32;
constexpr int kLD = kBK + 4;          // padded LDS row: the 16 rows of a ds_read_b128 group land on 16 different 4-bank slots
constexpr int kStageLD = kBN + 4;
constexpr size_t kLdsBytes = (size_t)(2 * kBM * kLD + 2 * kBN * kLD) * sizeof(float);
static_assert(kBM * kStageLD <= 2 * kBM * kLD + 2 * kBN * kLD, "the accumulator stage reuses the operand buffers");

struct DgradStridedArgs {
    const float* dy;      // [N][Ho][Wo][dy_ld]
    const float* wt;      // [Cin][R][S][Cout]
    float* dx;            // [N][Hi][Wi][dx_ld]
    int64_t dy_ld, dx_ld;
    int N, Hi, Wi, Cin, Ho, Wo, Cout, R, S, pad_y, pad_x;
    int tiles_n;
    int first1, first2, first3;     // first block of grid slots 1 .. 3 (slot s holds phase p = 3 - s, p = 2 * py + px; multiples of 8)
};

// blocks b and b + 8 share an XCD: give every XCD a contiguous range of tiles (conv.hip)
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// one 32-deep K-step of a wave's 64 x 32 tile: fragment / MFMA order of conv.hip's mma_kstep<2, 1, 32>
__device__ __forceinline__ void mma_kstep(const float* __restrict__ As, const float* __restrict__ Bs, int a_row0, int b_row0, int lane,
                                          f32x16 (&acc)[2]) {
    const int li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int t = 0; t < kBK / 8; ++t) {
        float4 a[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const float4*>(As + (a_row0 + i * 32 + li) * kLD + t * 8 + lh * 4);
        const float4 b = *reinterpret_cast<const float4*>(Bs + (b_row0 + li) * kLD + t * 8 + lh * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float bv = e == 0 ? b.x : e == 1 ? b.y : e == 2 ? b.z : b.w;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float av = e == 0 ? a[i].x : e == 1 ? a[i].y : e == 2 ? a[i].z : a[i].w;
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i], 0, 0, 0);
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void dgrad_strided_kernel(DgradStridedArgs a) {
    constexpr int CPR = kBK / 4;         // float4 chunks per LDS row
    constexpr int RPP = 256 / CPR;       // rows staged per pass of the block
    constexpr int NPA = kBM / RPP, NPB = kBN / RPP;
    extern __shared__ __align__(16) float smem[];
    float* As = smem;                    // [2][kBM][kLD]: dy rows of the current tap
    float* Bs = smem + 2 * kBM * kLD;    // [2][kBN][kLD]: the tap's [Cin][Cout] slice of the transpose
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = wv >> 1, wn = wv & 1;

    // Phase and tile of this block.  The four phases cost 1 : 2 : 2 : 4 K-steps per tile (3x3 / pad 1), so the grid holds them longest
    // first (slot s = phase 3 - s: the long blocks start first), each in a range padded to a multiple of 8 blocks: inside a range
    // block & 7 is the XCD, xcd_remap hands every XCD a contiguous run of that phase's tiles, and every XCD gets the same mix of
    // phases (one remap over the whole grid would give two XCDs nothing but four-tap tiles).  Blocks of the padding leave at once.
    const int b = blockIdx.x;
    const int slot = (b >= a.first1) + (b >= a.first2) + (b >= a.first3);
    const int first = slot == 3 ? a.first3 : slot == 2 ? a.first2 : slot == 1 ? a.first1 : 0;
    const int next = slot == 3 ? (int)gridDim.x : slot == 2 ? a.first3 : slot == 1 ? a.first2 : a.first1;
    const int p = 3 - slot;
    const int local = xcd_remap(b - first, next - first);
    const int py = p >> 1, px = p & 1;
    const int Hp = (a.Hi - py + 1) >> 1, Wp = (a.Wi - px + 1) >> 1;
    const int HpWp = Hp * Wp, Mp = a.N * HpWp;
    const int r0 = (py + a.pad_y) & 1, s0 = (px + a.pad_x) & 1;
    const int Rp = (a.R - r0 + 1) >> 1, Sp = (a.S - s0 + 1) >> 1;
    const int oy = (py + a.pad_y - r0) >> 1, ox = (px + a.pad_x - s0) >> 1;
    const int tile_n = local % a.tiles_n, tile_m = local / a.tiles_n;
    const int m0 = tile_m * kBM, n0 = tile_n * kBN;
    if (m0 >= Mp) return;                // (uniform over the block, before the first barrier)

    // loader geometry: thread owns column chunk c4 (4 floats) of rows lr + RPP * i
    const int lr = t / CPR, c4 = (t % CPR) * 4;
    int pixbase[NPA], jy[NPA], ix0[NPA];
    bool mok[NPA];
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        const int m = m0 + lr + RPP * i;
        mok[i] = m < Mp;
        const int mm = mok[i] ? m : 0;
        const int img = mm / HpWp, rem = mm - img * HpWp;
        const int j = rem / Wp;
        pixbase[i] = img * a.Ho * a.Wo;
        jy[i] = j + oy;
        ix0[i] = rem - j * Wp + ox;
    }
    const int RS = a.R * a.S;
    const int cchunks = a.Cout / kBK;
    const int ksteps = Rp * Sp * cchunks;

    // Branch-free loader: taps outside dy / rows beyond Mp / channels beyond Cin read a clamped (valid) address and are zeroed
    // by a multiply at LDS-store time.
    float4 ra[NPA], rb[NPB];
    float fa[NPA], fb[NPB];
    int cob[NPB];
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
        const int ci = n0 + lr + RPP * i;
        const bool cok = ci < a.Cin;
        cob[i] = cok ? ci : a.Cin - 1;
        fb[i] = cok ? 1.f : 0.f;
    }
    auto gload = [&](int ks) {
        const int tap = ks / cchunks, k0 = (ks - tap * cchunks) * kBK;
        const int tr = tap / Sp, ts = tap - tr * Sp;
        const int wtap = (r0 + 2 * tr) * a.S + s0 + 2 * ts;
#pragma unroll
        for (int i = 0; i < NPA; ++i) {
            const int iy = jy[i] - tr, ix = ix0[i] - ts;
            const bool ok = (unsigned)iy < (unsigned)a.Ho && (unsigned)ix < (unsigned)a.Wo && mok[i];
            const int cy = min(max(iy, 0), a.Ho - 1), cx = min(max(ix, 0), a.Wo - 1);
            const float* q = a.dy + (int64_t)(pixbase[i] + cy * a.Wo + cx) * a.dy_ld + k0 + c4;
            ra[i] = *reinterpret_cast<const float4*>(q);
            fa[i] = ok ? 1.f : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
            const float* q = a.wt + ((int64_t)cob[i] * RS + wtap) * a.Cout + k0 + c4;
            rb[i] = *reinterpret_cast<const float4*>(q);
        }
    };
    auto lstore = [&](int buf) {
        float* ad = As + buf * kBM * kLD;
        float* bd = Bs + buf * kBN * kLD;
#pragma unroll
        for (int i = 0; i < NPA; ++i)
            *reinterpret_cast<float4*>(ad + (lr + RPP * i) * kLD + c4) =
                make_float4(ra[i].x * fa[i], ra[i].y * fa[i], ra[i].z * fa[i], ra[i].w * fa[i]);
#pragma unroll
        for (int i = 0; i < NPB; ++i)
            *reinterpret_cast<float4*>(bd + (lr + RPP * i) * kLD + c4) =
                make_float4(rb[i].x * fb[i], rb[i].y * fb[i], rb[i].z * fb[i], rb[i].w * fb[i]);
    };

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    if (ksteps > 0) {                    // (uniform over the block: a phase without taps only stores its zeros)
        gload(0);
        lstore(0);
    }
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
        const int cur = ks & 1;
        if (ks + 1 < ksteps) gload(ks + 1);
        mma_kstep(As + cur * kBM * kLD, Bs + cur * kBN * kLD, wm * 64, wn * 32, lane, acc);
        if (ks + 1 < ksteps) lstore(cur ^ 1);
        __syncthreads();
    }

    // epilogue: the 128 x 64 tile goes through LDS (the operand buffers are free) and leaves in 16-byte pieces, 256 contiguous bytes per
    // pixel; accumulator register e of a 32x32 tile is row (e&3) + 8*(e>>2) + 4*(lane>>5), col lane&31.  Row m of the phase is pixel
    // (img, 2j + py, 2i + px) of dx.
    float* stage = smem;                 // [kBM][kStageLD]
    {
        const int li = lane & 31, lh = lane >> 5;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                stage[(wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * kStageLD + wn * 32 + li] = acc[i][e];
    }
    __syncthreads();
    constexpr int CQ = kBN / 4, RG = 256 / CQ, RPT = kBM / RG;
    const int cq = t % CQ, rg = t / CQ;
    const int n = n0 + cq * 4;
    if (n >= a.Cin) return;              // Cin % 4 == 0: a column quad is inside or outside as a whole
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int r = rg + RG * k;
        const int m = m0 + r;
        if (m < Mp) {
            const int img = m / HpWp, rem = m - img * HpWp;
            const int j = rem / Wp, i = rem - j * Wp;
            const float4 v = *reinterpret_cast<const float4*>(stage + r * kStageLD + cq * 4);
            float* o = a.dx + ((int64_t)(img * a.Hi + 2 * j + py) * a.Wi + 2 * i + px) * a.dx_ld + n;
            __builtin_nontemporal_store((f32x4nt){v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4nt*>(o));
        }
    }
}

}  // namespace
}  // namespace diga

using namespace diga;

extern "C" int diga_dgrad_strided_f32(const float* dy, int64_t dy_ld, const float* wgt_t, float* dx, int64_t dx_ld, int64_t N, int64_t Hi,
                                      int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y,
                                      int64_t stride_x, int64_t pad_y, int64_t pad_x, void* stream) {
    const char* who = "dgrad_strided";
    // the forward convolution's geometry in the terms of conv_call.h: input coordinate = out * stride + off0 + tap * off_d
    const int64_t off_y0 = -pad_y, off_x0 = -pad_x, off_dy = 1, off_dx = 1;
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = dy; c.in_ld = dy_ld; c.wgt = wgt_t; c.out = dx; c.out_ld = dx_ld; c.prof_tag = DIGA_PROF_CONV_BWD_DATA;

    DIGA_REQUIRE(dy && wgt_t && dx, DIGA_EINVAL, "%s: null pointer", who);
    DIGA_REQUIRE(aligned16(dy) && aligned16(wgt_t) && aligned16(dx), DIGA_EINVAL, "%s: pointers must be 16-byte aligned", who);
    DIGA_REQUIRE(c.stride_y == 2 && c.stride_x == 2, DIGA_EINVAL, "%s: stride %lld x %lld: only stride 2 x 2 is built", who,
                 (long long)c.stride_y, (long long)c.stride_x);
    DIGA_REQUIRE(c.N >= 0 && c.Hi > 0 && c.Wi > 0 && c.Cin > 0 && c.Cout > 0, DIGA_EINVAL, "%s: bad shape", who);
    DIGA_REQUIRE(c.Cout % 32 == 0, DIGA_EINVAL, "%s: Cout=%lld must be a multiple of 32 (the K-loop chunk)", who, (long long)c.Cout);
    DIGA_REQUIRE(c.Cin % 4 == 0, DIGA_EINVAL, "%s: Cin=%lld must be a multiple of 4", who, (long long)c.Cin);
    DIGA_REQUIRE(dy_ld >= c.Cout && dy_ld % 4 == 0, DIGA_EINVAL, "%s: bad dy_ld (>= Cout, %% 4 == 0)", who);
    DIGA_REQUIRE(dx_ld >= c.Cin && dx_ld % 4 == 0, DIGA_EINVAL, "%s: bad dx_ld (>= Cin, %% 4 == 0)", who);
    DIGA_REQUIRE(c.R >= 1 && c.R <= 7 && c.S >= 1 && c.S <= 7, DIGA_EINVAL, "%s: kernel extent %lld x %lld outside 1 .. 7", who,
                 (long long)c.R, (long long)c.S);
    DIGA_REQUIRE(pad_y >= 0 && pad_y < c.R && pad_x >= 0 && pad_x < c.S, DIGA_EINVAL, "%s: padding must be >= 0 and smaller than the kernel extent",
                 who);
    DIGA_REQUIRE(c.Hi + 2 * pad_y >= c.R && c.Wi + 2 * pad_x >= c.S && c.Ho == (c.Hi + 2 * pad_y - c.R) / 2 + 1 &&
                     c.Wo == (c.Wi + 2 * pad_x - c.S) / 2 + 1,
                 DIGA_EINVAL, "%s: Ho x Wo is not the stride-2 output extent of Hi x Wi (at least 1 x 1)", who);
    const int64_t lim = 1ll << 30;
    // (phase (0, 0) is the largest; each product's factors are bounded by the terms in front of it)
    DIGA_REQUIRE(c.N < lim && c.Hi < lim && c.Wi < lim && (c.Hi + 1) / 2 * ((c.Wi + 1) / 2) < lim &&
                     c.N * ((c.Hi + 1) / 2 * ((c.Wi + 1) / 2)) < lim && c.N * c.Ho < lim && c.N * c.Ho * c.Wo < 2 * lim,
                 DIGA_EINVAL, "%s: a phase's rows / pixel coordinates beyond 2^30", who);
    int rc = check_tap_coordinates(c, who);
    if (rc) return rc;
    if (c.N == 0) return DIGA_OK;

    DgradStridedArgs a;
    a.dy = dy; a.wt = wgt_t; a.dx = dx; a.dy_ld = dy_ld; a.dx_ld = dx_ld;
    a.N = (int)c.N; a.Hi = (int)c.Hi; a.Wi = (int)c.Wi; a.Cin = (int)c.Cin; a.Ho = (int)c.Ho; a.Wo = (int)c.Wo; a.Cout = (int)c.Cout;
    a.R = (int)c.R; a.S = (int)c.S; a.pad_y = (int)pad_y; a.pad_x = (int)pad_x;
    a.tiles_n = (int)ceil_div(c.Cin, kBN);
    int64_t first[5] = {0, 0, 0, 0, 0};
    for (int s = 0; s < 4; ++s) {      // slot s: phase 3 - s, its tile count rounded up to a multiple of 8 (see the kernel)
        const int p = 3 - s;
        const int64_t rows = c.N * ((c.Hi - (p >> 1) + 1) / 2) * ((c.Wi - (p & 1) + 1) / 2);
        first[s + 1] = first[s] + ceil_div(ceil_div(rows, kBM) * a.tiles_n, 8) * 8;
    }
    DIGA_REQUIRE(first[4] < (1ll << 31), DIGA_EINVAL, "%s: too many tiles for one launch", who);
    a.first1 = (int)first[1]; a.first2 = (int)first[2]; a.first3 = (int)first[3];

    hipStream_t st = (hipStream_t)c.stream;
    ProfScope prof(DIGA_PROF_CONV_BWD_DATA, st, 2.0 * (double)(c.N * c.Ho * c.Wo) * (double)c.Cout * (double)(c.R * c.S) * (double)c.Cin);
    (void)hipFuncSetAttribute((const void*)dgrad_strided_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    hipLaunchKernelGGL(dgrad_strided_kernel, dim3((unsigned)first[4]), dim3(256), kLdsBytes, st, a);
    return launch_status("diga_dgrad_strided_f32");
}
