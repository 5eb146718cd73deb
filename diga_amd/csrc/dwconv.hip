// Depthwise 3x3 convolution, stride 1, padding = dilation, fp32 NHWC with pitched operands: the depthwise half of the DAFormer head's
// separable ASPP branches (dilations 6 / 12 / 18 on the 1024-channel concatenation; diga_amd/model/networks/daformer_head.py).
//
//   y[n, i, j, c]  = sum_{r,s} w9[3r + s][c] * x[n, i + (r - 1) d, j + (s - 1) d, c]          zeros outside the map
//   dw9[t][c]      = sum_{n,i,j} dy[n, i, j, c] * x[n, i + (r - 1) d, j + (s - 1) d, c]       t = 3r + s
//
// and the backward-data pass is the first formula on dy with the taps reversed (`flip`: tap t reads weight 8 - t), so one kernel
// serves both.  9 multiply-adds per 8 bytes: there is nothing here for a matrix core, the passes are bandwidth passes (least traffic
// 8 B per element; the weight gradient reads 8 B per element and writes next to nothing), and all the design is about where the
// taps' re-reads come from.  The nine taps of a pixel sit up to 18 rows apart and one NHWC row of the head's geometry (192 pixels x
// 1024 channels) is 786 KB, so whole rows cannot stay in an XCD's 4 MiB L2; a 32-channel chunk of a row is 24 KB.  Hence:
//   * a block owns ONE row of ONE 32-channel chunk (thread = channel quad t % 8, pixel lane t / 8: 128 contiguous bytes per pixel,
//     16-byte loads along the channel axis) and walks the row 32 pixels at a time, nine independent loads in flight per step;
//   * the grid is ordered chunk-major, then image, then row, and xcd_remap hands every XCD a contiguous run of that order (blocks b
//     and b + 8 share an XCD): the blocks an XCD runs together are neighbouring rows of the same chunk, whose taps are each other's rows.
// The nine products of an output are added in tap order in one fmaf chain from 0; a tap outside the map enters as an exact 0, so a
// map that only the centre tap reaches gives w9[4] * x in fp32 bits.  Exact fp32 whatever conv_math is (DESIGN section 17's rule).
//
// Weight gradient: the same blocks over four rows each keep nine float4 sums per thread, fold the 32 pixel lanes (shuffles inside a
// wave, the four waves through LDS, fixed order) and write one [9][32] partial per block into the caller's workspace
// ([N * ceil(H / 4)][9][C]); a second kernel adds the partials of a (tap, channel) in block order.  No atomics: the bits do not depend
// on the run.
#include "common.h"

namespace diga {
namespace {

constexpr int kCQ = 8;            // channel quads per block: 32 channels
constexpr int kPL = 32;           // pixel lanes per block
constexpr int kWgRows = 4;        // rows per block of the weight-gradient kernel

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// blocks b and b + 8 share an XCD: give every XCD a contiguous range of the block order (conv.hip)
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

struct DwArgs {
    const float* x;       // [N][H][W][x_ld]
    const float* w9;      // [9][C]
    float* y;             // [N][H][W][y_ld]
    int64_t x_ld, y_ld;
    int N, H, W, C, d, flip;
};

__global__ __launch_bounds__(256) void dwconv3x3_kernel(DwArgs a) {
    const int t = threadIdx.x, q = t % kCQ, pl = t / kCQ;
    const int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int rows = a.N * a.H;
    const int chunk = b / rows, row = b - chunk * rows;
    const int n = row / a.H, i = row - n * a.H;
    const int c = (chunk * kCQ + q) * 4;
    if (c >= a.C) return;                         // C % 4 == 0: a quad is inside or outside as a whole (no barrier below)
    float4 w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = ld4(a.w9 + (int64_t)(a.flip ? 8 - k : k) * a.C + c);
    const float* img = a.x + (int64_t)n * a.H * a.W * a.x_ld + c;
    float* out = a.y + ((int64_t)n * a.H + i) * a.W * a.y_ld + c;
    int iy[3];
    bool rok[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        iy[r] = i + (r - 1) * a.d;
        rok[r] = (unsigned)iy[r] < (unsigned)a.H;
    }
    for (int j = pl; j < a.W; j += kPL) {
        float4 v[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int jx = j + (s - 1) * a.d;
                v[3 * r + s] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (rok[r] && (unsigned)jx < (unsigned)a.W) v[3 * r + s] = ld4(img + ((int64_t)iy[r] * a.W + jx) * a.x_ld);
            }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            acc.x = fmaf(w[k].x, v[k].x, acc.x);
            acc.y = fmaf(w[k].y, v[k].y, acc.y);
            acc.z = fmaf(w[k].z, v[k].z, acc.z);
            acc.w = fmaf(w[k].w, v[k].w, acc.w);
        }
        *reinterpret_cast<float4*>(out + (int64_t)j * a.y_ld) = acc;
    }
}

struct DwWgradArgs {
    const float* dy;      // [N][H][W][dy_ld]
    const float* x;       // [N][H][W][x_ld]
    float* part;          // [N * groups][9][C]
    int64_t dy_ld, x_ld;
    int N, H, W, C, d, groups;      // groups = ceil(H / kWgRows)
};

__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(DwWgradArgs a) {
    __shared__ float4 red[4][9][kCQ];             // 4.5 KB
    const int t = threadIdx.x, q = t % kCQ, pl = t / kCQ;
    const int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int per_chunk = a.N * a.groups;
    const int chunk = b / per_chunk, g = b - chunk * per_chunk;
    const int n = g / a.groups, i0 = (g - n * a.groups) * kWgRows;
    const int c = (chunk * kCQ + q) * 4;
    const bool cok = c < a.C;
    float4 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok) {
        const float* ximg = a.x + (int64_t)n * a.H * a.W * a.x_ld + c;
        const float* gimg = a.dy + (int64_t)n * a.H * a.W * a.dy_ld + c;
        const int i1 = min(i0 + kWgRows, a.H);
        for (int i = i0; i < i1; ++i) {
            int iy[3];
            bool rok[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                iy[r] = i + (r - 1) * a.d;
                rok[r] = (unsigned)iy[r] < (unsigned)a.H;
            }
            for (int j = pl; j < a.W; j += kPL) {
                const float4 gv = ld4(gimg + ((int64_t)i * a.W + j) * a.dy_ld);
                float4 v[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        const int jx = j + (s - 1) * a.d;
                        v[3 * r + s] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (rok[r] && (unsigned)jx < (unsigned)a.W) v[3 * r + s] = ld4(ximg + ((int64_t)iy[r] * a.W + jx) * a.x_ld);
                    }
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    acc[k].x = fmaf(gv.x, v[k].x, acc[k].x);
                    acc[k].y = fmaf(gv.y, v[k].y, acc[k].y);
                    acc[k].z = fmaf(gv.z, v[k].z, acc[k].z);
                    acc[k].w = fmaf(gv.w, v[k].w, acc[k].w);
                }
            }
        }
    }
    // the 8 pixel lanes of a wave that share a quad are lanes q, q + 8, ..., q + 56: fold bits 3..5, then the 4 waves through LDS
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) {
            acc[k].x += __shfl_xor(acc[k].x, o, 64);
            acc[k].y += __shfl_xor(acc[k].y, o, 64);
            acc[k].z += __shfl_xor(acc[k].z, o, 64);
            acc[k].w += __shfl_xor(acc[k].w, o, 64);
        }
    const int wv = t >> 6;
    if ((t & 63) < kCQ) {
#pragma unroll
        for (int k = 0; k < 9; ++k) red[wv][k][q] = acc[k];
    }
    __syncthreads();
    if (t < 9 * kCQ) {
        const int k = t / kCQ, qq = t % kCQ;
        const int cc = (chunk * kCQ + qq) * 4;
        if (cc < a.C) {
            float4 s = red[0][k][qq];
#pragma unroll
            for (int w4 = 1; w4 < 4; ++w4) {
                const float4 s2 = red[w4][k][qq];
                s.x += s2.x, s.y += s2.y, s.z += s2.z, s.w += s2.w;
            }
            *reinterpret_cast<float4*>(a.part + ((int64_t)g * 9 + k) * a.C + cc) = s;
        }
    }
}

// dw9[k][c] = the partials of (k, c) added in block order; one thread per (tap, channel quad)
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw9, int parts,
                                                                     int C) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int n4 = 9 * (C / 4);
    if (idx >= n4) return;
    const float* p = part + (int64_t)idx * 4;
    const int64_t step = (int64_t)9 * C;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int g = 0; g < parts; ++g) {
        const float4 v = ld4(p + g * step);
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
    *reinterpret_cast<float4*>(dw9 + (int64_t)idx * 4) = s;
}

// true where the elements [p, p + rows * ld) x [0, C) of the two pitched operands can share an address: the byte ranges overlap and the
// operands are not two disjoint column windows of one matrix (same pitch, offset a whole number of floats)
bool may_alias(const float* a, int64_t a_ld, const float* b, int64_t b_ld, int64_t rows, int64_t C) {
    if (rows <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t a1 = a0 + (uintptr_t)(((rows - 1) * a_ld + C) * 4), b1 = b0 + (uintptr_t)(((rows - 1) * b_ld + C) * 4);
    if (a1 <= b0 || b1 <= a0) return false;
    if (a_ld == b_ld) {
        const int64_t diff = (int64_t)((b0 > a0 ? b0 - a0 : a0 - b0) / 4) % a_ld;      // column offset of the later window in the earlier one's rows
        if (diff >= C && diff + C <= a_ld) return false;
    }
    return true;
}

constexpr int64_t kLim = 1ll << 30;
constexpr int64_t kMaxElems = 1ll << 44;      // pixels x pitch of one operand

}  // namespace
}  // namespace diga

using namespace diga;

extern "C" int diga_dwconv3x3_f32(const float* x, int64_t x_ld, const float* w9, float* y, int64_t y_ld, int64_t N, int64_t H, int64_t W,
                                  int64_t C, int64_t dilation, int flip, void* stream) {
    const char* who = "dwconv3x3";
    DIGA_REQUIRE(x && w9 && y, DIGA_EINVAL, "%s: null pointer", who);
    DIGA_REQUIRE(aligned16(x) && aligned16(w9) && aligned16(y), DIGA_EINVAL, "%s: pointers must be 16-byte aligned", who);
    DIGA_REQUIRE(N >= 0 && H > 0 && W > 0 && C > 0 && N < kLim && H < kLim && W < kLim && C < kLim, DIGA_EINVAL, "%s: bad shape", who);
    DIGA_REQUIRE(C % 4 == 0, DIGA_EINVAL, "%s: C=%lld must be a multiple of 4", who, (long long)C);
    DIGA_REQUIRE(x_ld >= C && x_ld % 4 == 0 && x_ld < kLim, DIGA_EINVAL, "%s: bad x_ld (>= C, %% 4 == 0, < 2^30)", who);
    DIGA_REQUIRE(y_ld >= C && y_ld % 4 == 0 && y_ld < kLim, DIGA_EINVAL, "%s: bad y_ld (>= C, %% 4 == 0, < 2^30)", who);
    DIGA_REQUIRE(dilation >= 1 && dilation < kLim, DIGA_EINVAL, "%s: dilation=%lld must be >= 1", who, (long long)dilation);
    DIGA_REQUIRE(flip == 0 || flip == 1, DIGA_EINVAL, "%s: flip is 0 or 1", who);
    const int64_t blocks = ceil_div(C, 4 * kCQ) * N * H;
    DIGA_REQUIRE(N * H < kLim && blocks < (1ll << 31), DIGA_EINVAL, "%s: too many rows for one launch", who);
    // (N * H < 2^30 and W < 2^30: the pixel count fits; with it below 2^44 / ld every byte offset below, may_alias's included, fits int64)
    DIGA_REQUIRE(N * H * W <= kMaxElems / x_ld && N * H * W <= kMaxElems / y_ld, DIGA_EINVAL, "%s: an operand beyond 2^44 elements", who);
    DIGA_REQUIRE(!may_alias(x, x_ld, y, y_ld, N * H * W, C), DIGA_EINVAL, "%s: x and y must not alias", who);
    if (N == 0) return DIGA_OK;
    DwArgs a;
    a.x = x; a.w9 = w9; a.y = y; a.x_ld = x_ld; a.y_ld = y_ld;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.C = (int)C; a.d = (int)dilation; a.flip = flip;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(DIGA_PROF_ELEMENTWISE, st, (double)N * H * W * C * 8.0);
    hipLaunchKernelGGL(dwconv3x3_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return launch_status("diga_dwconv3x3_f32");
}

extern "C" size_t diga_dwconv3x3_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || N >= kLim || H >= kLim || W >= kLim || C >= kLim) return 0;
    return (size_t)(N * ceil_div(H, kWgRows)) * 9 * (size_t)C * sizeof(float);
}

extern "C" int diga_dwconv3x3_f32_wgrad(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw9, void* workspace,
                                        size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t dilation,
                                        void* stream) {
    const char* who = "dwconv3x3_wgrad";
    DIGA_REQUIRE(dy && x && dw9 && workspace, DIGA_EINVAL, "%s: null pointer", who);
    DIGA_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(dw9) && aligned16(workspace), DIGA_EINVAL, "%s: pointers must be 16-byte aligned",
                 who);
    DIGA_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && N < kLim && H < kLim && W < kLim && C < kLim, DIGA_EINVAL, "%s: bad shape", who);
    DIGA_REQUIRE(C % 4 == 0, DIGA_EINVAL, "%s: C=%lld must be a multiple of 4", who, (long long)C);
    DIGA_REQUIRE(dy_ld >= C && dy_ld % 4 == 0 && dy_ld < kLim, DIGA_EINVAL, "%s: bad dy_ld (>= C, %% 4 == 0, < 2^30)", who);
    DIGA_REQUIRE(x_ld >= C && x_ld % 4 == 0 && x_ld < kLim, DIGA_EINVAL, "%s: bad x_ld (>= C, %% 4 == 0, < 2^30)", who);
    DIGA_REQUIRE(dilation >= 1 && dilation < kLim, DIGA_EINVAL, "%s: dilation=%lld must be >= 1", who, (long long)dilation);
    const int64_t groups = ceil_div(H, kWgRows), parts = N * groups;
    const int64_t blocks = ceil_div(C, 4 * kCQ) * parts;
    DIGA_REQUIRE(parts < kLim && blocks < (1ll << 31), DIGA_EINVAL, "%s: too many rows for one launch", who);
    DIGA_REQUIRE(N * H < kLim && N * H * W <= kMaxElems / dy_ld && N * H * W <= kMaxElems / x_ld, DIGA_EINVAL,
                 "%s: an operand beyond 2^44 elements", who);
    const size_t need = diga_dwconv3x3_wgrad_workspace_bytes(N, H, W, C);
    DIGA_REQUIRE(workspace_bytes >= need, DIGA_EINVAL, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    DwWgradArgs a;
    a.dy = dy; a.x = x; a.part = (float*)workspace; a.dy_ld = dy_ld; a.x_ld = x_ld;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.C = (int)C; a.d = (int)dilation; a.groups = (int)groups;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(DIGA_PROF_ELEMENTWISE, st, (double)N * H * W * C * 8.0);
    hipLaunchKernelGGL(dwconv3x3_wgrad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(dwconv3x3_wgrad_reduce_kernel, dim3((unsigned)ceil_div(9 * (C / 4), 256)), dim3(256), 0, st, (const float*)workspace, dw9,
                       (int)parts, (int)C);
    return launch_status("diga_dwconv3x3_f32_wgrad");
}
