// "bf16x6": fp32-equivalent pointwise (1x1) convolutions on the bf16 matrix cores (DIGA_CONV_MATH_BF16X6).
// Included at the end of conv.hip: it reuses that file's ConvArgs / WgradArgs, drain_stage (bias, BatchNorm statistics, the
// backward-data epilogue), the transposing fragment reads, the pixel table and the fixed-order slab reduce.
//
// Arithmetic.  An fp32 value a is carried EXACTLY as three bf16 planes (3 x 8 = 24 significand bits):
//     a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1)         (round to nearest even; the subtractions are exact)
// and a product of two such values as six of the nine plane products, smallest first, with fp32 accumulation:
//     a1 b1 + a0 b2 + a2 b0 + a0 b1 + a1 b0 + a0 b0                     (a1 b2, a2 b1, a2 b2 <= 2^-24 of the product: dropped)
// on v_mfma_f32_16x16x32_bf16.  tools/bf16x6_emulation.py is the host restatement (and its error against float64).
// Non-finite inputs: a0 keeps the inf / nan and a - a0 is nan, so the result is nan where exact fp32 might give inf.
// Inputs below 2^-110 in magnitude: the low planes leave bf16's normal range and lose bits (they may flush to zero), the
// sum of the planes is then no longer the input; relative to any activation or weight of normal size that is < 2^-100.
//
// Accumulator scheme ("fold"): per 16 x 16 sub-tile and 32-deep K-step the five correction terms are chained from a ZERO
// accumulator (they are <= 2^-8 of the leading term, so their roundings are 2^-8 smaller too), the leading product a0 b0
// goes into the persistent accumulator, and one VALU add folds the corrections in: two roundings of the running sum per
// K-step instead of six.  Chosen over two persistent accumulator sets because 2 x 64 accumulator registers do not fit the
// 168-register budget of three waves per SIMD next to 48 registers of weight fragments; it costs 4 temporaries per
// sub-tile in flight.  The host emulation puts it at 1.0e-7 .. 5.7e-7 of scale for K = 64 .. 2048, under the per-k fp32
// chain's 3.1e-7 .. 1.8e-6; tests/test_gpu_conv_bf16x6.py holds it to the exact-fp32 kernels measured on the device.
//
// Operands are split ONCE per call by two elementwise passes and then staged global -> LDS by LDS-DMA loads, as in the
// two-plane "twin" family (conv_fwd_x3t8_kernel / conv_wgrad_x3t_kernel) whose skeleton these kernels keep:
//   * activations as a "triplet" image: per pixel and group of 8 channels 16 B of plane 0, 16 B of plane 1, 16 B of
//     plane 2 (6 B per element), make_triplet_kernel;
//   * weights as three-plane LDS images per output-channel tile and K-step, swizzled as they sit in LDS
//     (split_image3_kernel).
// Tile and ring: 256 x (64*TN) x 32 per block as in the twin kernel; a three-plane stage is 72 KB at TN = 2, so the ring
// has TWO stages (144 KB of the 160 KB LDS) where the twin kernel has three: the loads of K-step k + 1 are in flight
// while step k's 96 MFMAs per wave issue.  Built that way the forward kernel takes 152 / 154 VGPRs (plain / backward-data
// epilogue) with no spill, the weight-gradient kernel 238 of its 256.  Measured (tools/bench_conv.py, 16 images of 768 x 768,
// profiles/r07_bf16x6_bench_conv.txt): 1024 -> 2048 channels forward 3.37 ms against 4.80 ms exact fp32 (187 against 131
// TFLOP/s, split passes included), weight gradient 3.13 against 4.80 ms; count-weighted over the model's pointwise layers
// forward 53.0 / backward-data 52.2 / weight gradient 40.4 ms against 56.2 / 54.9 / 54.6 ms.  What it does NOT win: the
// triplet pass reads 4 B and writes 6 B per element at HBM speed (28 % of a 1024 -> 256 layer's forward), so a forward with
// Cin >= 4 Cout, a backward-data with Cout >= 4 Cin and every layer of layer1 / layer2 is slower than exact fp32 in that one
// pass (DESIGN.md section 8 has the table).  Not tuned beyond this.
#pragma once

namespace diga {

// 4 fp32 -> 3 x 4 bf16 (planes 0, 1, 2)
__device__ __forceinline__ void split3x4(const float4 v, uint2& p0, uint2& p1, uint2& p2) {
    p0.x = pack_bf16(v.x, v.y);
    p0.y = pack_bf16(v.z, v.w);
    const float r0 = v.x - __uint_as_float(p0.x << 16), r1 = v.y - __uint_as_float(p0.x & 0xffff0000u);
    const float r2 = v.z - __uint_as_float(p0.y << 16), r3 = v.w - __uint_as_float(p0.y & 0xffff0000u);
    p1.x = pack_bf16(r0, r1);
    p1.y = pack_bf16(r2, r3);
    const float s0 = r0 - __uint_as_float(p1.x << 16), s1 = r1 - __uint_as_float(p1.x & 0xffff0000u);
    const float s2 = r2 - __uint_as_float(p1.y << 16), s3 = r3 - __uint_as_float(p1.y & 0xffff0000u);
    p2.x = pack_bf16(s0, s1);
    p2.y = pack_bf16(s2, s3);
}

// x [M][ld] fp32 (C channels) -> triplet [M][C/8][plane0 x 8 | plane1 x 8 | plane2 x 8]
__global__ __launch_bounds__(256) void make_triplet_kernel(const float* __restrict__ x, int64_t ld, unsigned char* __restrict__ trip,
                                                           int64_t M, int C8) {
    const int64_t total = M * C8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / C8;
        const int g = (int)(i - m * C8);
        const float* src = x + m * ld + g * 8;
        uint2 a0, a1, a2, b0, b1, b2;
        split3x4(*reinterpret_cast<const float4*>(src), a0, a1, a2);
        split3x4(*reinterpret_cast<const float4*>(src + 4), b0, b1, b2);
        uint4* dst = reinterpret_cast<uint4*>(trip + i * 48);
        dst[0] = make_uint4(a0.x, a0.y, b0.x, b0.y);
        dst[1] = make_uint4(a1.x, a1.y, b1.x, b1.y);
        dst[2] = make_uint4(a2.x, a2.y, b2.x, b2.y);
    }
}

// Weights [K][RS][C] fp32 -> LDS images: for every tile of `bn` output channels and every 32-channel K-step (tap-major)
// 3 * bn * 64 bytes = plane 0, plane 1, plane 2, one 64-byte row per output channel (rows past K repeat the last
// channel: never stored), the four 16-byte k-slots of row r at slot ^ lds_swz(r)  (split_image_kernel with a third plane).
__global__ __launch_bounds__(256) void split_image3_kernel(const float* __restrict__ w, unsigned char* __restrict__ img,
                                                           int K, int RS, int C, int bn, int64_t total) {
    const int cchunks = C / 32, ksteps = RS * cchunks;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int s = (int)(i & 3);
        const int r = (int)((i >> 2) % bn);
        const int64_t tk = (i >> 2) / bn;               // tile * ksteps + ks
        const int ks = (int)(tk % ksteps), tile = (int)(tk / ksteps);
        const int tap = ks / cchunks, cc = ks - tap * cchunks;
        const int n = min(tile * bn + r, K - 1);
        const float* src = w + ((int64_t)n * RS + tap) * C + cc * 32 + 8 * s;
        uint2 a0, a1, a2, b0, b1, b2;
        split3x4(*reinterpret_cast<const float4*>(src), a0, a1, a2);
        split3x4(*reinterpret_cast<const float4*>(src + 4), b0, b1, b2);
        const int64_t plane = (int64_t)bn * 64;
        unsigned char* dst = img + tk * (3 * plane) + r * 64 + ((s ^ lds_swz(r)) << 4);
        *reinterpret_cast<uint4*>(dst) = make_uint4(a0.x, a0.y, b0.x, b0.y);
        *reinterpret_cast<uint4*>(dst + plane) = make_uint4(a1.x, a1.y, b1.x, b1.y);
        *reinterpret_cast<uint4*>(dst + 2 * plane) = make_uint4(a2.x, a2.y, b2.x, b2.y);
    }
}

// split_image3_kernel on `gridDim.y` stacked weight arrays (the Winograd-domain U [batches][K][C], RS = 1): batch b reads
// w + b * w_stride floats and writes img + b * img_stride bytes -- each image byte for byte what the kernel above makes of U_b.
__global__ __launch_bounds__(256) void split_image3_batched_kernel(const float* __restrict__ w, unsigned char* __restrict__ img,
                                                                   int K, int C, int bn, int64_t total, int64_t w_stride,
                                                                   int64_t img_stride) {
    const int ksteps = C / 32;
    w += (int64_t)blockIdx.y * w_stride;
    img += (int64_t)blockIdx.y * img_stride;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int s = (int)(i & 3);
        const int r = (int)((i >> 2) % bn);
        const int64_t tk = (i >> 2) / bn;               // tile * ksteps + ks
        const int ks = (int)(tk % ksteps), tile = (int)(tk / ksteps);
        const int n = min(tile * bn + r, K - 1);
        const float* src = w + (int64_t)n * C + ks * 32 + 8 * s;
        uint2 a0, a1, a2, b0, b1, b2;
        split3x4(*reinterpret_cast<const float4*>(src), a0, a1, a2);
        split3x4(*reinterpret_cast<const float4*>(src + 4), b0, b1, b2);
        const int64_t plane = (int64_t)bn * 64;
        unsigned char* dst = img + tk * (3 * plane) + r * 64 + ((s ^ lds_swz(r)) << 4);
        *reinterpret_cast<uint4*>(dst) = make_uint4(a0.x, a0.y, b0.x, b0.y);
        *reinterpret_cast<uint4*>(dst + plane) = make_uint4(a1.x, a1.y, b1.x, b1.y);
        *reinterpret_cast<uint4*>(dst + 2 * plane) = make_uint4(a2.x, a2.y, b2.x, b2.y);
    }
}

#define DIGA_LDS_DMA16(src_, dst_)                                                                   \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src_),         \
                                     (__attribute__((address_space(3))) void*)(dst_), 16, 0, 0)

// ---------------------------------------------------------------------------------------------
// forward / backward-data of a 1x1 convolution (any stride, offsets (oy0, ox0)): 12 waves = 8 MFMA waves as 4 (M) x 2 (N),
// wave tile 64 x (32*TN), + 4 LDS-DMA loader waves; two-stage ring, one raw barrier per K-step (barrier k + 1 says both
// "step k's MFMAs are done" and "stage k + 1 has landed").  Epilogue = conv_fwd_x3t8_kernel's (drain_stage).
// ---------------------------------------------------------------------------------------------
//
// LS ("loader split", the `_f32in` entry points): a.in is the fp32 tensor itself ([pixel][in_ld], a channel slice of a wider
// NHWC buffer included).  The loader lanes keep their rows, their k-slot and their 16-byte LDS slot; per row a lane reads its 8
// channels as two float4 (a wave instruction covers 16 rows x 128 contiguous bytes), runs split3x4 -- the pass form's function, so
// the planes are the same bits -- and writes the three planes with ds_write_b128 where the DMA form lands them.  The LDS image is
// byte-identical: MFMA waves, fold accumulator and drain_stage are shared.  Weights stay pre-split images staged by LDS-DMA.
// Schedule per K-step: loads of step k + 1 into registers + the weight DMA, vmcnt(0), split, ds_write, lgkmcnt(0), barrier (the
// stage written was last read in step k - 1, behind the previous barrier).  No triplet pass and 4 instead of 6 B per element
// through L2; the price is ~6 VALU instructions per element in the loader waves.
//
// WB ("weight batches", the Winograd-domain GEMMs: gemm_batched_bf16x6): the rows are `batches` stacked products of a.wb_tiles row
// tiles each and row tile tile_m takes its weight image from batch tile_m / a.wb_tiles (a.wb_stride BYTES between the images; the
// fp32 kernels use the two fields the same way, in floats).  Rows per batch are a multiple of 256, so no tile straddles two
// batches; rows, slots, swizzle, ring, K-step order, MFMA waves and drain_stage are the un-batched kernel's -- so are a tile's bits.
//
// INF (the `_infer` entry points): the staged tile leaves through the inference epilogue of diga_infer_epilogue_t (drain_stage's INF
// form, infer_rows; TAG = 1: this family's own instantiations of it) -- an instantiation of its own, so the others keep their registers.  Nothing before the drain reads it: the
// accumulator that reaches the stage is the plain kernel's, bit for bit.
//
// TAPS (the `diga_conv_taps_*` entry points; LS only): a convolution with R * S <= 64 taps at offsets (oy0 + r * ody, ox0 + q * odx),
// any sign (backward-data negates them), any stride.  The K-steps are (live taps) x Cin / 32, tap-major -- the order of
// split_image3_kernel's image (ks = tap * cchunks + cc), so an R x S layer runs the K-step sequence of the pointwise kernel on the
// tap-major im2col rows [M][RS * Cin] of its input: same weight image bytes, same LDS bytes, same bits.  Taps that lie outside the
// image for every row of the block's tile (live_taps: uniform over the block) are stepped over in the weight image: they would add
// exact zeros.  The loader lanes keep rows, k-slot, swizzle, LDS slot and the issue / vmcnt(0) / split3x4 / ds_write_b128 /
// lgkmcnt(0) / barrier schedule; per row they keep the image's first pixel and (y0, x0) = (ho * sy + oy0, wo * sx + ox0), per tap they
// derive (y0 + r * ody, x0 + q * odx) and the pointer -- null outside the image: no load is issued, the planes written are zero.  The
// MFMA waves learn the new K-step count and nothing else; drain_stage, the fold accumulator and the ring are untouched.
template <int TN, bool EPI = false, bool LS = false, bool WB = false, bool INF = false, bool TAPS = false>
__global__ __launch_bounds__(768, 3) void conv_fwd_x6_kernel(ConvArgs a) {
    static_assert(!(INF && (EPI || WB)), "the inference epilogue comes with the plain pointwise forward");
    static_assert(!TAPS || (LS && !WB), "the tap walk lives in the loader-split form");
    constexpr int BM = 256, BN = 64 * TN, NT = 2 * TN, MT = 4;
    constexpr int A_PLANE = BM * 64, B_PLANE = BN * 64, STAGE = 3 * A_PLANE + 3 * B_PLANE;
    extern __shared__ __align__(16) unsigned char smem_b[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool loader = wv >= 8;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_n = wg % a.tiles_n, tile_m = wg / a.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    int ksteps_all = a.Cin / 32;
    uint64_t live = 0;
    if constexpr (TAPS) {
        live = live_taps(a, m0, BM);                             // (never empty)
        ksteps_all *= __builtin_popcountll(live);
    }
    const int ksteps = ksteps_all;

    if constexpr (TAPS) {
      if (loader) {
        const int lw = wv - 8;                                   // 0..3: A rows lw*64 + 16 j + (lane >> 2)
        const int lrow = lane >> 2;
        const int kslot = (lane & 3) ^ lds_swz(lrow);
        const int HoWo = a.Ho * a.Wo, cchunks = a.Cin / 32;
        int pix0[4], y0[4], x0[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = min(m0 + lw * 64 + 16 * j + lrow, a.M - 1);
            const int img = m / HoWo, rem = m - img * HoWo;
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            pix0[j] = img * a.Hi * a.Wi;
            y0[j] = ho * a.sy + a.oy0;
            x0[j] = wo * a.sx + a.ox0;
        }
        const float* pa[4];
        uint64_t todo = live;
        int l_tap = 0, l_cc = 0, issued = 0;
        auto next_tap = [&]() {                                  // -> l_tap = the next live tap, pa = its pixels
            l_tap = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int r = l_tap / a.S, q = l_tap - r * a.S;
            const int dy = r * a.ody, dx = q * a.odx;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iy = y0[j] + dy, ix = x0[j] + dx;
                const bool ok = (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
                pa[j] = ok ? a.in + ((int64_t)pix0[j] + (int64_t)iy * a.Wi + ix) * a.in_ld + kslot * 8 : nullptr;
            }
        };
        const unsigned char* bimg = a.wgt_img + (int64_t)tile_n * ((int64_t)a.R * a.S * cchunks) * (3 * B_PLANE) + (lw * 3 * TN) * 1024 + lane * 16;
        float4 v[4][2];
        auto issue = [&](int buf) {                              // global loads of the next K-step into registers + its weight DMA
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pa[j] != nullptr) {
                    v[j][0] = *reinterpret_cast<const float4*>(pa[j] + l_cc * 32);
                    v[j][1] = *reinterpret_cast<const float4*>(pa[j] + l_cc * 32 + 4);
                }
            }
            const unsigned char* bsrc = bimg + (int64_t)(l_tap * cchunks + l_cc) * (3 * B_PLANE);
            unsigned char* bdst = smem_b + buf * STAGE + 3 * A_PLANE + (lw * 3 * TN) * 1024;
#pragma unroll
            for (int c = 0; c < 3 * TN; ++c) DIGA_LDS_DMA16(bsrc + c * 1024, bdst + c * 1024);
        };
        auto write = [&](int buf) {                              // split + three ds_write_b128 per row, wait for them, step on
            unsigned char* stage = smem_b + buf * STAGE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;     // a pixel outside the image: zero planes
                if (pa[j] != nullptr) {
                    uint2 a0, a1, a2, b0, b1, b2;
                    split3x4(v[j][0], a0, a1, a2);
                    split3x4(v[j][1], b0, b1, b2);
                    q0 = make_uint4(a0.x, a0.y, b0.x, b0.y);
                    q1 = make_uint4(a1.x, a1.y, b1.x, b1.y);
                    q2 = make_uint4(a2.x, a2.y, b2.x, b2.y);
                }
                unsigned char* dst = stage + (lw * 64 + 16 * j) * 64 + lane * 16;
                *reinterpret_cast<uint4*>(dst) = q0;
                *reinterpret_cast<uint4*>(dst + A_PLANE) = q1;
                *reinterpret_cast<uint4*>(dst + 2 * A_PLANE) = q2;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ++issued;
            if (++l_cc == cchunks) {                             // (pa changes only here, behind the writes that read it)
                l_cc = 0;
                if (issued < ksteps) next_tap();
            }
        };
        next_tap();
        issue(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        write(0);
        __builtin_amdgcn_s_barrier();                            // stage 0 has landed
        for (int ks = 0; ks < ksteps; ++ks) {
            if (ks + 1 < ksteps) {                               // (its stage was read by step ks - 1: behind the last barrier)
                issue((ks + 1) & 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                write((ks + 1) & 1);
            }
            __builtin_amdgcn_s_barrier();
        }
        return;
      }
    } else if constexpr (LS) {
      if (loader) {
        const int lw = wv - 8;                                   // 0..3: A rows lw*64 + 16 j + (lane >> 2)
        const int lrow = lane >> 2;
        const int kslot = (lane & 3) ^ lds_swz(lrow);
        const int HoWo = a.Ho * a.Wo;
        const float* pa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = min(m0 + lw * 64 + 16 * j + lrow, a.M - 1);
            const int img = m / HoWo, rem = m - img * HoWo;
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            const int iy = ho * a.sy + a.oy0, ix = wo * a.sx + a.ox0;
            const bool ok = (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
            pa[j] = ok ? a.in + ((int64_t)img * a.Hi * a.Wi + (int64_t)iy * a.Wi + ix) * a.in_ld + kslot * 8 : nullptr;
        }
        const unsigned char* wimg = a.wgt_img;
        if constexpr (WB) wimg += (int64_t)(tile_m / a.wb_tiles) * a.wb_stride;
        const unsigned char* bimg = wimg + (int64_t)tile_n * ksteps * (3 * B_PLANE) + (lw * 3 * TN) * 1024 + lane * 16;
        float4 v[4][2];
        auto issue = [&](int ks, int buf) {                      // global loads of step ks into registers + its weight DMA
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pa[j] != nullptr) {
                    v[j][0] = *reinterpret_cast<const float4*>(pa[j] + ks * 32);
                    v[j][1] = *reinterpret_cast<const float4*>(pa[j] + ks * 32 + 4);
                }
            }
            const unsigned char* bsrc = bimg + (int64_t)ks * (3 * B_PLANE);
            unsigned char* bdst = smem_b + buf * STAGE + 3 * A_PLANE + (lw * 3 * TN) * 1024;
#pragma unroll
            for (int c = 0; c < 3 * TN; ++c) DIGA_LDS_DMA16(bsrc + c * 1024, bdst + c * 1024);
        };
        auto write = [&](int buf) {                              // split + three ds_write_b128 per row, then wait for them
            unsigned char* stage = smem_b + buf * STAGE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;     // a pixel outside the image: zero planes
                if (pa[j] != nullptr) {
                    uint2 a0, a1, a2, b0, b1, b2;
                    split3x4(v[j][0], a0, a1, a2);
                    split3x4(v[j][1], b0, b1, b2);
                    q0 = make_uint4(a0.x, a0.y, b0.x, b0.y);
                    q1 = make_uint4(a1.x, a1.y, b1.x, b1.y);
                    q2 = make_uint4(a2.x, a2.y, b2.x, b2.y);
                }
                unsigned char* dst = stage + (lw * 64 + 16 * j) * 64 + lane * 16;
                *reinterpret_cast<uint4*>(dst) = q0;
                *reinterpret_cast<uint4*>(dst + A_PLANE) = q1;
                *reinterpret_cast<uint4*>(dst + 2 * A_PLANE) = q2;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        };
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        write(0);
        __builtin_amdgcn_s_barrier();                            // stage 0 has landed
        for (int ks = 0; ks < ksteps; ++ks) {
            if (ks + 1 < ksteps) {                               // (its stage was read by step ks - 1: behind the last barrier)
                issue(ks + 1, (ks + 1) & 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                write((ks + 1) & 1);
            }
            __builtin_amdgcn_s_barrier();
        }
        return;
      }
    } else if (loader) {
        const int lw = wv - 8;                                   // 0..3: A rows lw*64 + 16 j + (lane >> 2)
        const unsigned char* trip = reinterpret_cast<const unsigned char*>(a.in);
        const int lrow = lane >> 2;
        const int kslot = (lane & 3) ^ lds_swz(lrow);
        const int64_t rowb = (int64_t)a.Cin * 6;
        const int HoWo = a.Ho * a.Wo;
        const unsigned char* pa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = min(m0 + lw * 64 + 16 * j + lrow, a.M - 1);
            const int img = m / HoWo, rem = m - img * HoWo;
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            const int iy = ho * a.sy + a.oy0, ix = wo * a.sx + a.ox0;
            const bool ok = (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
            pa[j] = ok ? trip + ((int64_t)img * a.Hi * a.Wi + (int64_t)iy * a.Wi + ix) * rowb + kslot * 48 : nullptr;
        }
        const unsigned char* bimg = a.wgt_img + (int64_t)tile_n * ksteps * (3 * B_PLANE) + (lw * 3 * TN) * 1024 + lane * 16;
        auto issue = [&](int ks, int buf) {
            unsigned char* stage = smem_b + buf * STAGE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = pa[j] != nullptr;
                const unsigned char* src = ok ? pa[j] + ks * 192 : g_zero16;          // 4 groups of 8 channels x 48 B
                unsigned char* dst = stage + (lw * 64 + 16 * j) * 64;
                DIGA_LDS_DMA16(src, dst);
                DIGA_LDS_DMA16(ok ? src + 16 : g_zero16, dst + A_PLANE);
                DIGA_LDS_DMA16(ok ? src + 32 : g_zero16, dst + 2 * A_PLANE);
            }
            const unsigned char* bsrc = bimg + (int64_t)ks * (3 * B_PLANE);
            unsigned char* bdst = stage + 3 * A_PLANE + (lw * 3 * TN) * 1024;
#pragma unroll
            for (int c = 0; c < 3 * TN; ++c) DIGA_LDS_DMA16(bsrc + c * 1024, bdst + c * 1024);
        };
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                            // stage 0 has landed
        for (int ks = 0; ks < ksteps; ++ks) {
            if (ks + 1 < ksteps) issue(ks + 1, (ks + 1) & 1);    // (its stage was read by step ks - 1: behind the last barrier)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        return;
    }

    const int wm = wv >> 1, wn = wv & 1;                          // 4 x 2 MFMA waves
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15;
    const int foff = frow * 64 + (((lane >> 4) ^ lds_swz(frow)) << 4);
    const int aoff = wm * 64 * 64 + foff;
    const int boff = 3 * A_PLANE + wn * 32 * TN * 64 + foff;

    __builtin_amdgcn_s_barrier();                                // stage 0 has landed
    for (int ks = 0; ks < ksteps; ++ks) {
        const unsigned char* A0 = smem_b + (ks & 1) * STAGE + aoff;
        const unsigned char* B0 = smem_b + (ks & 1) * STAGE + boff;
        bf16x8_t b0[NT], b1[NT], b2[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            b0[j] = *reinterpret_cast<const bf16x8_t*>(B0 + j * 1024);
            b1[j] = *reinterpret_cast<const bf16x8_t*>(B0 + B_PLANE + j * 1024);
            b2[j] = *reinterpret_cast<const bf16x8_t*>(B0 + 2 * B_PLANE + j * 1024);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const bf16x8_t a0 = *reinterpret_cast<const bf16x8_t*>(A0 + i * 1024);
            const bf16x8_t a1 = *reinterpret_cast<const bf16x8_t*>(A0 + A_PLANE + i * 1024);
            const bf16x8_t a2 = *reinterpret_cast<const bf16x8_t*>(A0 + 2 * A_PLANE + i * 1024);
            f32x4 t[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) t[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[j], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) t[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b2[j], t[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) t[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0[j], t[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) t[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1[j], t[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) t[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0[j], t[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] += t[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    __syncthreads();                                             // (8 surviving waves) everyone is out of the ring

    // epilogue: thread group h = wv >> 2 (waves 4h .. 4h+3 = rows 128h .. 128h+127) stages and drains its half
    constexpr int LDS_LD = BN + 4;
    const int h = wv >> 2, t = threadIdx.x & 255;
    float* stage = reinterpret_cast<float*>(smem_b) + h * (128 * LDS_LD);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                stage[((wm & 1) * 64 + i * 16 + (lane >> 4) * 4 + e) * LDS_LD + wn * 32 * TN + j * 16 + (lane & 15)] = acc[i][j][e];
    __syncthreads();
    if constexpr (INF) drain_stage<2, TN, false, 256, true, 1>(stage, a, m0 + h * 128, n0, t, tile_m * 2 + h, m0 + h * 128 < a.M);
    else drain_stage<2, TN, EPI>(stage, a, m0 + h * 128, n0, t, tile_m * 2 + h, m0 + h * 128 < a.M);
}

// ---------------------------------------------------------------------------------------------
// backward-weight on the triplets of dy and x: conv_wgrad_x3t_kernel with a third plane, six products in the order above
// with the fold accumulator, and a two-stage ring (72 KB stages).  256 (Cout) x 128 (Cin) tile per pixel range; four
// MFMA waves (wave tile 128 x 64) + four loader waves; fragments through the transposing LDS reads.
// ---------------------------------------------------------------------------------------------
//
// LS (diga_conv2d_wgrad_bf16x6_f32in): dy and x are the fp32 tensors ([pixel][dy_ld] / [pixel][x_ld]); the loader lanes keep row,
// destination chunk, source-side swizzle and clamps, read their chunk's 8 channels as two float4, split (split3x4) and write the
// three planes into the lane-linear LDS slots of the DMA form -- the same LDS bytes, so the same dw bits.
//
// WB (wgrad_batched_bf16x6, the Winograd-domain weight gradient): `R * S` independent products dU_b = Z_b^T V_b, the batch riding
// on the tap index as in conv_wgrad_dma_kernel -- tap b reads dy + b * a.dy_tap_stride and x + b * a.x_tap_stride (a.M rows each),
// the pixel table is the identity (a.ptab is null and not read), and a block's pixel range is clamped (dy) and zero-filled (x)
// within its batch's a.M rows.  The store is the un-batched one: slab [Cout][batches][Cin].
template <bool LS = false, bool WB = false>
__global__ __launch_bounds__(512, 1) void conv_wgrad_x6_kernel(WgradArgs a) {
    constexpr int BM = 256, BN = 128, MT = 8, NT = 4;
    constexpr int A_ROW = BM * 2, B_ROW = BN * 2;                       // bytes per pixel row and plane
    constexpr int A_PLANE = kBK * A_ROW, B_PLANE = kBK * B_ROW, STAGE = 3 * A_PLANE + 3 * B_PLANE;   // 72 KB
    extern __shared__ __align__(16) unsigned char smem_b[];
    const int t = threadIdx.x & 255, lane = t & 63, wv = t >> 6;
    const bool loader = threadIdx.x >= 256;
    const int wm = wv >> 1, wn = wv & 1;
    const int RS = a.R * a.S;
    int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_n = wg % a.tiles_n;
    wg /= a.tiles_n;
    const int tile_m = wg % a.tiles_m;
    wg /= a.tiles_m;
    const int tap = wg % RS;
    const int split = wg / RS;
    const int k0 = tile_m * BM, c0 = tile_n * BN;
    const int p_begin = split * a.steps_per_split * kBK;
    int p_end = p_begin + a.steps_per_split * kBK;
    if (p_end > a.M) p_end = a.M;
    const int ksteps = p_end > p_begin ? (p_end - p_begin + kBK - 1) / kBK : 0;

    if constexpr (LS) {
      if (loader) {
        const int* tab = WB ? nullptr : a.ptab + (int64_t)tap * a.M_pad;
        const float* dyb = a.dy;
        const float* xb = a.x;
        if constexpr (WB) {
            dyb += (int64_t)tap * a.dy_tap_stride;
            xb += (int64_t)tap * a.x_tap_stride;
        }
        const int a_chunk_dst = lane & 31, b_chunk_dst = lane & 15;
        const int kgrp = k0 / 8, cgrp = c0 / 8, kmax = a.Cout / 8 - 1, cmax = a.Cin / 8 - 1;
        float4 va[4][2], vb[2][2];
        bool okb[2];
        auto issue = [&](int ks) {                          // global loads of step ks into registers
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 8 * wv + 2 * j + (lane >> 5);
                const int p = min(p_begin + ks * kBK + row, a.M - 1);
                const int chunk = min(kgrp + (a_chunk_dst ^ (tr_key(row) << 1)), kmax);
                const float* src = dyb + (int64_t)p * a.dy_ld + chunk * 8;
                va[j][0] = *reinterpret_cast<const float4*>(src);
                va[j][1] = *reinterpret_cast<const float4*>(src + 4);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = 8 * wv + 4 * j + (lane >> 4);
                const int p = p_begin + ks * kBK + row;
                int xi = -1;
                if (p < p_end) {
                    if constexpr (WB) xi = p;
                    else xi = tab[p];
                }
                okb[j] = xi >= 0;
                if (okb[j]) {
                    const int chunk = min(cgrp + (b_chunk_dst ^ (tr_key(row) << 1)), cmax);
                    const float* src = xb + (int64_t)xi * a.x_ld + chunk * 8;
                    vb[j][0] = *reinterpret_cast<const float4*>(src);
                    vb[j][1] = *reinterpret_cast<const float4*>(src + 4);
                }
            }
        };
        auto write = [&](int stg) {                         // split + ds_write_b128 of the three planes, then wait for them
            unsigned char* stage = smem_b + stg * STAGE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint2 a0, a1, a2, b0, b1, b2;
                split3x4(va[j][0], a0, a1, a2);
                split3x4(va[j][1], b0, b1, b2);
                unsigned char* dst = stage + (8 * wv + 2 * j) * A_ROW + lane * 16;
                *reinterpret_cast<uint4*>(dst) = make_uint4(a0.x, a0.y, b0.x, b0.y);
                *reinterpret_cast<uint4*>(dst + A_PLANE) = make_uint4(a1.x, a1.y, b1.x, b1.y);
                *reinterpret_cast<uint4*>(dst + 2 * A_PLANE) = make_uint4(a2.x, a2.y, b2.x, b2.y);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;     // outside the image / past the pixel range: zero planes
                if (okb[j]) {
                    uint2 a0, a1, a2, b0, b1, b2;
                    split3x4(vb[j][0], a0, a1, a2);
                    split3x4(vb[j][1], b0, b1, b2);
                    q0 = make_uint4(a0.x, a0.y, b0.x, b0.y);
                    q1 = make_uint4(a1.x, a1.y, b1.x, b1.y);
                    q2 = make_uint4(a2.x, a2.y, b2.x, b2.y);
                }
                unsigned char* dst = stage + 3 * A_PLANE + (8 * wv + 4 * j) * B_ROW + lane * 16;
                *reinterpret_cast<uint4*>(dst) = q0;
                *reinterpret_cast<uint4*>(dst + B_PLANE) = q1;
                *reinterpret_cast<uint4*>(dst + 2 * B_PLANE) = q2;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        };
        if (ksteps > 0) {
            issue(0);
            write(0);
        }
        __builtin_amdgcn_s_barrier();                      // stage 0 has landed
        for (int ks = 0; ks < ksteps; ++ks) {
            if (ks + 1 < ksteps) {                         // (its stage was read by step ks - 1: behind the last barrier)
                issue(ks + 1);
                write((ks + 1) & 1);
            }
            __builtin_amdgcn_s_barrier();
        }
        return;
      }
    } else if (loader) {
        const unsigned char* dyt = reinterpret_cast<const unsigned char*>(a.dy);
        const unsigned char* xt = reinterpret_cast<const unsigned char*>(a.x);
        const int64_t dy_rowb = (int64_t)a.Cout * 6, x_rowb = (int64_t)a.Cin * 6;
        const int* tab = a.ptab + (int64_t)tap * a.M_pad;
        // A (dy): 32 rows x 32 chunks per plane = 16 LDS-DMA instructions, 4 per wave: instruction j of wave wv covers
        //         rows 8 wv + 2 j + (lane >> 5), destination chunk lane & 31.   B (x): 32 rows x 16 chunks = 8
        //         instructions per plane, 2 per wave: rows 8 wv + 4 j + (lane >> 4), destination chunk lane & 15.
        const int a_chunk_dst = lane & 31, b_chunk_dst = lane & 15;
        const int kgrp = k0 / 8, cgrp = c0 / 8, kmax = a.Cout / 8 - 1, cmax = a.Cin / 8 - 1;
        auto issue = [&](int ks, int stg) {
            unsigned char* stage = smem_b + stg * STAGE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 8 * wv + 2 * j + (lane >> 5);
                const int p = min(p_begin + ks * kBK + row, a.M - 1);
                const int chunk = min(kgrp + (a_chunk_dst ^ (tr_key(row) << 1)), kmax);
                const unsigned char* src = dyt + p * dy_rowb + (int64_t)chunk * 48;
                unsigned char* dst = stage + (8 * wv + 2 * j) * A_ROW;
                DIGA_LDS_DMA16(src, dst);
                DIGA_LDS_DMA16(src + 16, dst + A_PLANE);
                DIGA_LDS_DMA16(src + 32, dst + 2 * A_PLANE);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = 8 * wv + 4 * j + (lane >> 4);
                const int p = p_begin + ks * kBK + row;
                const int xi = p < p_end ? tab[p] : -1;
                const bool ok = xi >= 0;
                const int chunk = min(cgrp + (b_chunk_dst ^ (tr_key(row) << 1)), cmax);
                const unsigned char* src = ok ? xt + xi * x_rowb + (int64_t)chunk * 48 : g_zero16;
                unsigned char* dst = stage + 3 * A_PLANE + (8 * wv + 4 * j) * B_ROW;
                DIGA_LDS_DMA16(src, dst);
                DIGA_LDS_DMA16(ok ? src + 16 : g_zero16, dst + B_PLANE);
                DIGA_LDS_DMA16(ok ? src + 32 : g_zero16, dst + 2 * B_PLANE);
            }
        };
        if (ksteps > 0) issue(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // stage 0 has landed
        for (int ks = 0; ks < ksteps; ++ks) {
            if (ks + 1 < ksteps) issue(ks + 1, (ks + 1) & 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        return;
    }

    // ---------------------------------------------------------------------- MFMA waves
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // transposing read of this lane (conv_wgrad_x3t_kernel): group g = lane >> 4 takes pixel rows 8 g + q (+ 4 for the second read)
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int row0 = 8 * g + q, row1 = row0 + 4;
    const int key0 = tr_key(row0) << 1, key1 = tr_key(row1) << 1;
    auto a_off = [&](int tile, int row, int key) { return row * A_ROW + (((2 * (wm * 8 + tile) + (pp >> 1)) ^ key) << 4) + ((pp & 1) << 3); };
    auto b_off = [&](int tile, int row, int key) { return row * B_ROW + (((2 * (wn * 4 + tile) + (pp >> 1)) ^ key) << 4) + ((pp & 1) << 3); };

    __builtin_amdgcn_s_barrier();                          // stage 0 has landed
    for (int ks = 0; ks < ksteps; ++ks) {
        const unsigned char* Ap = smem_b + (ks & 1) * STAGE;
        const unsigned char* Bp = Ap + 3 * A_PLANE;
        bf16x8_t b0[NT], b1[NT], b2[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            b0[j] = tr_frag(Bp + b_off(j, row0, key0), Bp + b_off(j, row1, key1));
            b1[j] = tr_frag(Bp + B_PLANE + b_off(j, row0, key0), Bp + B_PLANE + b_off(j, row1, key1));
            b2[j] = tr_frag(Bp + 2 * B_PLANE + b_off(j, row0, key0), Bp + 2 * B_PLANE + b_off(j, row1, key1));
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const bf16x8_t a0 = tr_frag(Ap + a_off(i, row0, key0), Ap + a_off(i, row1, key1));
            const bf16x8_t a1 = tr_frag(Ap + A_PLANE + a_off(i, row0, key0), Ap + A_PLANE + a_off(i, row1, key1));
            const bf16x8_t a2 = tr_frag(Ap + 2 * A_PLANE + a_off(i, row0, key0), Ap + 2 * A_PLANE + a_off(i, row1, key1));
            f32x4 tt[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) tt[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[j], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) tt[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b2[j], tt[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) tt[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0[j], tt[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) tt[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1[j], tt[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) tt[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0[j], tt[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] += tt[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    float* out = a.slab + (int64_t)split * a.Cout * RS * a.Cin;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = c0 + wn * 64 + j * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = k0 + wm * 128 + i * 16 + (lane >> 4) * 4 + e;
                if (kk < a.Cout && c < a.Cin) out[((int64_t)kk * RS + tap) * a.Cin + c] = acc[i][j][e];
            }
        }
    }
}

#undef DIGA_LDS_DMA16

}  // namespace diga

// ---- C ABI (include/diga_hip.h, "bf16x6")
extern "C" int diga_make_triplet(const float* x, int64_t ld, void* triplet, int64_t M, int64_t C, void* stream) {
    DIGA_REQUIRE(x && triplet && M > 0 && C > 0 && C % 8 == 0 && ld >= C && ld % 4 == 0, DIGA_EINVAL, "make_triplet: C must be a multiple of 8");
    DIGA_REQUIRE(aligned16(x) && aligned16(triplet), DIGA_EALIGN, "make_triplet: pointers must be 16-byte aligned");
    int64_t blocks = ceil_div(M * (C / 8), 256);
    if (blocks > 16384) blocks = 16384;
    ProfScope prof(DIGA_PROF_ELEMENTWISE, (hipStream_t)stream, (double)M * C * 10.0);
    hipLaunchKernelGGL(make_triplet_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ld, (unsigned char*)triplet, M,
                       (int)(C / 8));
    return launch_status("diga_make_triplet");
}

extern "C" size_t diga_split_bf16x6_image_bytes(int64_t K, int64_t RS, int64_t C) {
    if (K <= 0 || RS <= 0 || C <= 0 || C % 32 != 0) return 0;
    const int64_t bn = image_bn(K);
    return (size_t)(ceil_div(K, bn) * RS * (C / 32) * 3 * bn * 64);
}

extern "C" int diga_split_bf16x6_image(const float* w, void* img, int64_t K, int64_t RS, int64_t C, void* stream) {
    DIGA_REQUIRE(w && img && K > 0 && RS > 0 && C > 0 && C % 32 == 0, DIGA_EINVAL, "split_bf16x6_image: C must be a multiple of 32");
    DIGA_REQUIRE(aligned16(w) && aligned16(img), DIGA_EALIGN, "split_bf16x6_image: pointers must be 16-byte aligned");
    const int64_t bn = image_bn(K);
    const int64_t total = ceil_div(K, bn) * RS * (C / 32) * bn * 4;
    int64_t blocks = ceil_div(total, 256);
    if (blocks > 8192) blocks = 8192;
    ProfScope prof(DIGA_PROF_ELEMENTWISE, (hipStream_t)stream, (double)K * RS * C * 10.0);
    hipLaunchKernelGGL(split_image3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, (unsigned char*)img, (int)K,
                       (int)RS, (int)C, (int)bn, total);
    return launch_status("diga_split_bf16x6_image");
}

// in_ld < 0: `in_triplet` is a triplet image (the pass form); else it is the fp32 tensor with that row pitch (the loader form).
// inf: the inference epilogue (the `_infer` entry points; forward without statistics and without a backward epilogue), checked by
// set_infer_epilogue -- the rules of diga_conv2d_nhwc_f32_infer -- before anything is launched.
static int conv2d_bf16x6_impl(const void* in_triplet, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N, int64_t Hi,
                              int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                              int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                              float* stats_partial, int prof_tag, void* stream, const diga_bwd_epilogue_t* epi,
                              const diga_infer_epilogue_t* inf = nullptr, bool taps = false) {
    DIGA_REQUIRE(in_triplet && wgt_img && out, DIGA_EINVAL, "conv2d_bf16x6: null pointer");
    DIGA_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && Cout > 0, DIGA_EINVAL, "conv2d_bf16x6: bad shape");
    if (taps) {
        // the `diga_conv_taps_*` entry points (loader form only): up to 64 taps (live_taps' mask), every coordinate the loader
        // derives -- (Ho - 1) * stride + offset + (R - 1) * step -- within 32 bits
        DIGA_REQUIRE(in_ld >= 0, DIGA_EINVAL, "conv_taps_bf16x6: in_ld must be at least Cin and a multiple of 4");
        DIGA_REQUIRE(R >= 1 && S >= 1 && R <= 64 && S <= 64 && R * S <= 64, DIGA_EINVAL, "conv_taps_bf16x6: 1 <= R * S <= 64 taps");
        DIGA_REQUIRE(stride_y > 0 && stride_x > 0, DIGA_EINVAL, "conv_taps_bf16x6: strides must be positive");
        const int64_t lim = 1ll << 30;
        DIGA_REQUIRE(stride_y < lim && stride_x < lim && off_y0 > -lim && off_y0 < lim && off_x0 > -lim && off_x0 < lim && off_dy > -lim &&
                     off_dy < lim && off_dx > -lim && off_dx < lim && Ho * stride_y < lim && Wo * stride_x < lim &&
                     (off_dy < 0 ? -off_dy : off_dy) * R < lim && (off_dx < 0 ? -off_dx : off_dx) * S < lim,
                     DIGA_EINVAL, "conv_taps_bf16x6: strides / offsets beyond 32-bit pixel coordinates");
    } else {
        DIGA_REQUIRE(R == 1 && S == 1 && stride_y > 0 && stride_x > 0, DIGA_EINVAL, "conv2d_bf16x6: pointwise (1x1) convolutions only");
    }
    DIGA_REQUIRE(Cin > 0 && Cin % 32 == 0 && out_ld >= Cout, DIGA_EINVAL, "conv2d_bf16x6: Cin must be a multiple of 32");
    const bool f32in = in_ld >= 0;
    DIGA_REQUIRE(!f32in || (in_ld >= Cin && in_ld % 4 == 0 && in_ld < (1ll << 31)), DIGA_EINVAL,
                 "conv2d_bf16x6_f32in: in_ld must be at least Cin and a multiple of 4");
    DIGA_REQUIRE(aligned16(in_triplet) && aligned16(wgt_img) && ((uintptr_t)out & 3u) == 0, DIGA_EALIGN, "conv2d_bf16x6: alignment");
    DIGA_REQUIRE(N * Hi * Wi < (1ll << 31) && N * Ho * Wo < (1ll << 31), DIGA_EINVAL, "conv2d_bf16x6: too many pixels");
    // every output pixel reads an input pixel inside the image or zeros: the loader checks the coordinate, so any
    // (stride, offset) is in bounds
    ConvArgs a;
    a.in = reinterpret_cast<const float*>(in_triplet); a.wgt = nullptr; a.wgt_hi = nullptr; a.wgt_lo = nullptr;
    a.wgt_img = reinterpret_cast<const unsigned char*>(wgt_img); a.bias = bias; a.out = out; a.stats = stats_partial;
    a.N = (int)N; a.Hi = (int)Hi; a.Wi = (int)Wi; a.Cin = (int)Cin; a.in_ld = f32in ? (int)in_ld : (int)Cin;
    a.Ho = (int)Ho; a.Wo = (int)Wo; a.Cout = (int)Cout; a.out_ld = (int)out_ld;
    a.R = (int)R; a.S = (int)S; a.sy = (int)stride_y; a.sx = (int)stride_x;
    a.oy0 = (int)off_y0; a.ox0 = (int)off_x0; a.ody = (int)off_dy; a.odx = (int)off_dx;
    a.M = (int)(N * Ho * Wo);
    a.tiles_m = (int)ceil_div(a.M, 256);
    a.all_inside = 0;
    const int tn = Cout > 64 ? 2 : 1;                 // (= image_bn(Cout) / 64: the weight image's tile)
    a.tiles_n = (int)ceil_div(Cout, 64 * tn);
    DIGA_REQUIRE(!taps || (int64_t)a.tiles_m * a.tiles_n < (1ll << 31), DIGA_EINVAL, "conv_taps_bf16x6: too many tiles for one launch");
    set_options(a, nullptr);
    {
        int rc = set_bwd_epilogue(a, epi, "conv2d_bf16x6");
        if (rc) return rc;
        rc = set_infer_epilogue(a, inf, "conv2d_bf16x6_infer");
        if (rc) return rc;
        DIGA_REQUIRE(!inf || (!epi && prof_tag != DIGA_PROF_CONV_BWD_DATA), DIGA_EINVAL,
                     "conv2d_bf16x6_infer: the inference epilogue comes with the forward (no backward epilogue)");
    }
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(prof_tag == DIGA_PROF_CONV_BWD_DATA ? DIGA_PROF_CONV_BWD_DATA : DIGA_PROF_CONV_FWD, st,
                   2.0 * (double)a.M * (double)Cout * (double)(R * S) * (double)Cin);
    const size_t ring = (size_t)2 * (3 * 256 * 64 + 3 * 64 * tn * 64);
    const size_t stg = (size_t)2 * 128 * (64 * tn + 4) * sizeof(float);
    const size_t sh = ring > stg ? ring : stg;
    if (taps) {
        if (inf != nullptr) {
            if (tn == 2) DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, false, true, false, true, true>), 768, sh);
            else DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, false, true, false, true, true>), 768, sh);
            return launch_status("diga_infer_conv_taps_bf16x6_f32in");
        }
        if (tn == 2) {
            if (epi != nullptr) DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, true, true, false, false, true>), 768, sh);
            else DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, false, true, false, false, true>), 768, sh);
        } else {
            if (epi != nullptr) DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, true, true, false, false, true>), 768, sh);
            else DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, false, true, false, false, true>), 768, sh);
        }
        return launch_status("diga_conv_taps_bf16x6_f32in");
    }
    if (inf != nullptr) {
        if (f32in) {
            if (tn == 2) DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, false, true, false, true>), 768, sh);
            else DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, false, true, false, true>), 768, sh);
            return launch_status("diga_infer_conv2d_nhwc_bf16x6_f32in");
        }
        if (tn == 2) DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, false, false, false, true>), 768, sh);
        else DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, false, false, false, true>), 768, sh);
        return launch_status("diga_infer_conv2d_nhwc_bf16x6");
    }
    if (f32in) {
        if (tn == 2) {
            if (epi != nullptr) DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, true, true>), 768, sh);
            else DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, false, true>), 768, sh);
        } else {
            if (epi != nullptr) DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, true, true>), 768, sh);
            else DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, false, true>), 768, sh);
        }
        return launch_status("diga_conv2d_nhwc_bf16x6_f32in");
    }
    if (tn == 2) {
        if (epi != nullptr) DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, true>), 768, sh);
        else DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, false>), 768, sh);
    } else {
        if (epi != nullptr) DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, true>), 768, sh);
        else DIGA_LAUNCH_K((conv_fwd_x6_kernel<1, false>), 768, sh);
    }
    return launch_status("diga_conv2d_nhwc_bf16x6");
}

extern "C" int diga_conv2d_nhwc_bf16x6(const void* in_triplet, const void* wgt_img, const float* bias, float* out, int64_t N,
                                       int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                       int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                       int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag, void* stream) {
    return conv2d_bf16x6_impl(in_triplet, -1, wgt_img, bias, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, stats_partial, prof_tag, stream, nullptr);
}

extern "C" int diga_conv2d_nhwc_bf16x6_epi(const void* in_triplet, const void* wgt_img, float* out, int64_t N, int64_t Hi, int64_t Wi,
                                           int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                                           int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy,
                                           int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag, void* stream) {
    DIGA_REQUIRE(epi != nullptr, DIGA_EINVAL, "conv2d_bf16x6_epi: null epilogue descriptor");
    return conv2d_bf16x6_impl(in_triplet, -1, wgt_img, nullptr, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, nullptr, prof_tag, stream, epi);
}

extern "C" int diga_conv2d_nhwc_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out,
                                             int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                             int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                             int64_t off_x0, int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag,
                                             void* stream) {
    DIGA_REQUIRE(in_ld >= 0, DIGA_EINVAL, "conv2d_bf16x6_f32in: in_ld must be at least Cin and a multiple of 4");
    return conv2d_bf16x6_impl(in, in_ld, wgt_img, bias, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, stats_partial, prof_tag, stream, nullptr);
}

extern "C" int diga_conv2d_nhwc_bf16x6_f32in_epi(const float* in, int64_t in_ld, const void* wgt_img, float* out, int64_t N, int64_t Hi,
                                                 int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                                 int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                                 int64_t off_x0, int64_t off_dy, int64_t off_dx, const diga_bwd_epilogue_t* epi,
                                                 int prof_tag, void* stream) {
    DIGA_REQUIRE(epi != nullptr, DIGA_EINVAL, "conv2d_bf16x6_f32in_epi: null epilogue descriptor");
    DIGA_REQUIRE(in_ld >= 0, DIGA_EINVAL, "conv2d_bf16x6_f32in_epi: in_ld must be at least Cin and a multiple of 4");
    return conv2d_bf16x6_impl(in, in_ld, wgt_img, nullptr, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, nullptr, prof_tag, stream, epi);
}

// The pointwise forward with the inference epilogue (include/diga_hip.h, diga_infer_epilogue_t): conv_fwd_x6_kernel<TN, ..., INF>.
extern "C" int diga_infer_conv2d_nhwc_bf16x6(const void* in_triplet, const void* wgt_img, const float* bias, float* out, int64_t N,
                                             int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                             int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                             int64_t off_dy, int64_t off_dx, const diga_infer_epilogue_t* infer, int prof_tag,
                                             void* stream) {
    DIGA_REQUIRE(infer != nullptr, DIGA_EINVAL, "conv2d_bf16x6_infer: null epilogue descriptor");
    return conv2d_bf16x6_impl(in_triplet, -1, wgt_img, bias, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, nullptr, prof_tag, stream, nullptr, infer);
}

extern "C" int diga_infer_conv2d_nhwc_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out,
                                                   int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                                   int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                                   int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                                   const diga_infer_epilogue_t* infer, int prof_tag, void* stream) {
    DIGA_REQUIRE(infer != nullptr, DIGA_EINVAL, "conv2d_bf16x6_f32in_infer: null epilogue descriptor");
    DIGA_REQUIRE(in_ld >= 0, DIGA_EINVAL, "conv2d_bf16x6_f32in_infer: in_ld must be at least Cin and a multiple of 4");
    return conv2d_bf16x6_impl(in, in_ld, wgt_img, bias, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, nullptr, prof_tag, stream, nullptr, infer);
}

// Multi-tap convolutions on the loader form (conv_fwd_x6_kernel<..., TAPS>): the argument lists of the pointwise `_f32in` entry
// points with 1 <= R * S <= 64; R = S = 1 gives the pointwise kernel's bits.
extern "C" int diga_conv_taps_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                           int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                           int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                           int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag, void* stream) {
    return conv2d_bf16x6_impl(in, in_ld, wgt_img, bias, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, stats_partial, prof_tag, stream, nullptr, nullptr, true);
}

extern "C" int diga_conv_taps_bf16x6_f32in_epi(const float* in, int64_t in_ld, const void* wgt_img, float* out, int64_t N, int64_t Hi,
                                               int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R,
                                               int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                               int64_t off_dy, int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag,
                                               void* stream) {
    DIGA_REQUIRE(epi != nullptr, DIGA_EINVAL, "conv_taps_bf16x6_f32in_epi: null epilogue descriptor");
    return conv2d_bf16x6_impl(in, in_ld, wgt_img, nullptr, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, nullptr, prof_tag, stream, epi, nullptr, true);
}

extern "C" int diga_infer_conv_taps_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out,
                                                 int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                                 int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                                 int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                                 const diga_infer_epilogue_t* infer, int prof_tag, void* stream) {
    DIGA_REQUIRE(infer != nullptr, DIGA_EINVAL, "infer_conv_taps_bf16x6_f32in: null epilogue descriptor");
    return conv2d_bf16x6_impl(in, in_ld, wgt_img, bias, out, N, Hi, Wi, Cin, Ho, Wo, Cout, out_ld, R, S, stride_y, stride_x, off_y0,
                              off_x0, off_dy, off_dx, nullptr, prof_tag, stream, nullptr, infer, true);
}

namespace {
// 256 x 128 tiles at one block per CU: about two rounds of 256 blocks, at least 8 K-steps (256 pixels) per block.  Short pixel
// ranges are also what keeps the weight gradient's error at the exact-fp32 kernels' level: the running sum of a range is
// rounded twice per K-step, the slabs are then added in fixed order by slab_reduce_kernel.  (plan_wgrad_wide, tuned for the
// widest layers, leaves a narrow layer on ONE block walking every pixel: measured 5x the fp32 kernel's error on a 64 -> 64
// layer over 37 636 pixels.)
// RS: independent products sharing the launch (the batched Winograd-domain form; 1 for a pointwise layer).
WgradPlan plan_wgrad_x6(int64_t M, int64_t Cout, int64_t Cin, int64_t RS = 1) {
    WgradPlan p;
    p.tm = 4;
    p.tn = 2;
    p.tiles_m = (int)ceil_div(Cout, 256);
    p.tiles_n = (int)ceil_div(Cin, 128);
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n * RS, ksteps = ceil_div(M, kBK);
    int64_t splits = ceil_div(512, tiles);
    const int64_t max_splits = ksteps / 8 > 0 ? ksteps / 8 : 1;
    if (splits > max_splits) splits = max_splits;
    if (splits > 512) splits = 512;
    p.steps_per_split = (int)ceil_div(ksteps, splits);
    p.splits = (int)ceil_div(ksteps, p.steps_per_split);
    return p;
}
// shape rules of the multi-tap weight gradient (shared by the entry point's checks and its workspace query)
bool taps_wgrad_shape_ok(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R, int64_t S) {
    const int64_t lim = 1ll << 31;
    if (N <= 0 || Ho <= 0 || Wo <= 0 || R < 1 || S < 1 || R > 64 || S > 64 || R * S > 64 || Cin <= 0 || Cin % 32 != 0 || Cin >= lim ||
        Cout <= 0 || Cout % 8 != 0 || Cout >= lim || N >= lim || Ho >= lim || Wo >= lim || N * Ho >= lim || N * Ho * Wo >= lim)
        return false;
    const WgradPlan p = plan_wgrad_x6(N * Ho * Wo, Cout, Cin, R * S);
    return ceil_div(Cout, 256) * ceil_div(Cin, 128) * R * S * p.splits < (1ll << 31);
}
}  // namespace

extern "C" size_t diga_conv2d_wgrad_bf16x6_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin,
                                                           int64_t R, int64_t S) {
    const int64_t M = N * Ho * Wo, RS = R * S;
    return wgrad_slab_bytes(plan_wgrad_x6(M, Cout, Cin), Cout, Cin, RS) + (size_t)RS * wgrad_mpad(M) * sizeof(int) + 64;
}

// dy_ld < 0: the operands are triplet images (the pass form); else the fp32 tensors with these row pitches (the loader form)
static int conv2d_wgrad_bf16x6_impl(const void* dy_triplet, int64_t dy_ld, const void* x_triplet, int64_t x_ld, float* dw,
                                    void* workspace, size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin,
                                    int64_t Ho, int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                    int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream,
                                    bool taps = false) {
    const bool f32in = dy_ld >= 0;
    DIGA_REQUIRE(dy_triplet && x_triplet && dw && workspace, DIGA_EINVAL, "conv2d_wgrad_bf16x6: null pointer");
    DIGA_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, DIGA_EINVAL, "conv2d_wgrad_bf16x6: bad shape");
    if (taps) {
        // diga_conv_taps_wgrad_bf16x6_f32in: one block group per tap from the pixel table of all taps (conv_wgrad_x6_kernel<true>)
        DIGA_REQUIRE(f32in && taps_wgrad_shape_ok(N, Ho, Wo, Cout, Cin, R, S) && stride_y > 0 && stride_x > 0, DIGA_EINVAL,
                     "conv_taps_wgrad_bf16x6: 1 <= R * S <= 64, Cin %% 32, Cout %% 8, positive strides and a block count below 2^31 required");
        const int64_t lim = 1ll << 30;
        DIGA_REQUIRE(stride_y < lim && stride_x < lim && off_y0 > -lim && off_y0 < lim && off_x0 > -lim && off_x0 < lim && off_dy > -lim &&
                     off_dy < lim && off_dx > -lim && off_dx < lim && Ho * stride_y < lim && Wo * stride_x < lim &&
                     (off_dy < 0 ? -off_dy : off_dy) * R < lim && (off_dx < 0 ? -off_dx : off_dx) * S < lim,
                     DIGA_EINVAL, "conv_taps_wgrad_bf16x6: strides / offsets beyond 32-bit pixel coordinates");
    } else {
        DIGA_REQUIRE(R == 1 && S == 1 && stride_y > 0 && stride_x > 0, DIGA_EINVAL, "conv2d_wgrad_bf16x6: pointwise (1x1) convolutions only");
    }
    DIGA_REQUIRE(Cin > 0 && Cin % 8 == 0 && Cout > 0 && Cout % 8 == 0, DIGA_EINVAL, "conv2d_wgrad_bf16x6: channel counts must be multiples of 8");
    DIGA_REQUIRE(!f32in || (dy_ld >= Cout && dy_ld % 4 == 0 && x_ld >= Cin && x_ld % 4 == 0 && dy_ld < (1ll << 31) && x_ld < (1ll << 31)),
                 DIGA_EINVAL, "conv2d_wgrad_bf16x6_f32in: dy_ld / x_ld must be at least the channel count and multiples of 4");
    DIGA_REQUIRE(aligned16(dy_triplet) && aligned16(x_triplet) && aligned16(dw) && aligned16(workspace), DIGA_EALIGN, "conv2d_wgrad_bf16x6: alignment");
    DIGA_REQUIRE(N * Hi * Wi < (1ll << 31) && N * Ho * Wo < (1ll << 31), DIGA_EINVAL, "conv2d_wgrad_bf16x6: too many pixels");
    const int64_t RS = taps ? R * S : 1, M = N * Ho * Wo, M_pad = wgrad_mpad(M);
    const WgradPlan p = plan_wgrad_x6(M, Cout, Cin, RS);
    const size_t slab_bytes = wgrad_slab_bytes(p, Cout, Cin, RS);
    DIGA_REQUIRE(workspace_bytes >= slab_bytes + (size_t)RS * M_pad * sizeof(int) + 64, DIGA_EWORKSPACE, "conv2d_wgrad_bf16x6: workspace too small");
    WgradArgs a;
    a.dy = reinterpret_cast<const float*>(dy_triplet); a.x = reinterpret_cast<const float*>(x_triplet);
    a.slab = p.splits > 1 ? (float*)workspace : dw;
    a.N = (int)N; a.Hi = (int)Hi; a.Wi = (int)Wi; a.Cin = (int)Cin; a.x_ld = f32in ? (int)x_ld : (int)Cin;
    a.Ho = (int)Ho; a.Wo = (int)Wo; a.Cout = (int)Cout; a.dy_ld = f32in ? (int)dy_ld : (int)Cout;
    a.R = taps ? (int)R : 1; a.S = taps ? (int)S : 1; a.sy = (int)stride_y; a.sx = (int)stride_x;
    a.oy0 = (int)off_y0; a.ox0 = (int)off_x0; a.ody = (int)off_dy; a.odx = (int)off_dx;
    a.M = (int)M; a.tiles_m = p.tiles_m; a.tiles_n = p.tiles_n; a.splits = p.splits; a.steps_per_split = p.steps_per_split;
    a.M_pad = (int)M_pad;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(DIGA_PROF_CONV_BWD_WEIGHT, st, 2.0 * (double)M * (double)Cout * (double)RS * (double)Cin);
    // (output pixel) -> input pixel table, -1 outside the image: in bounds for any stride / offset
    int* tab = reinterpret_cast<int*>(static_cast<char*>(workspace) + slab_bytes);
    float* zeros = reinterpret_cast<float*>(tab + RS * M_pad);
    hipLaunchKernelGGL(wgrad_pixtab_kernel, dim3((unsigned)ceil_div(M_pad, 256), (unsigned)RS), dim3(256), 0, st, tab, zeros, (int)M,
                       (int)M_pad, (int)Ho, (int)Wo, (int)Hi, (int)Wi, a.S, (int)stride_y, (int)stride_x, (int)off_y0, (int)off_x0,
                       (int)off_dy, (int)off_dx);
    a.ptab = tab;
    a.zeros = zeros;
    const unsigned grid = (unsigned)((int64_t)p.tiles_m * p.tiles_n * RS * p.splits);
    const size_t sh = (size_t)2 * (3 * kBK * 512 + 3 * kBK * 256);
    if (f32in) {
        (void)hipFuncSetAttribute((const void*)conv_wgrad_x6_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
        hipLaunchKernelGGL(conv_wgrad_x6_kernel<true>, dim3(grid), dim3(512), sh, st, a);
    } else {
        (void)hipFuncSetAttribute((const void*)conv_wgrad_x6_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
        hipLaunchKernelGGL(conv_wgrad_x6_kernel<false>, dim3(grid), dim3(512), sh, st, a);
    }
    if (p.splits > 1) {
        const int64_t n4 = Cout * RS * Cin / 4;
        hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0, st, (const float*)workspace, dw, n4,
                           p.splits);
    }
    return launch_status(taps ? "diga_conv_taps_wgrad_bf16x6_f32in" : f32in ? "diga_conv2d_wgrad_bf16x6_f32in" : "diga_conv2d_wgrad_bf16x6");
}

extern "C" int diga_conv2d_wgrad_bf16x6(const void* dy_triplet, const void* x_triplet, float* dw, void* workspace,
                                        size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho,
                                        int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                        int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream) {
    return conv2d_wgrad_bf16x6_impl(dy_triplet, -1, x_triplet, -1, dw, workspace, workspace_bytes, N, Hi, Wi, Cin, Ho, Wo, Cout, R, S,
                                    stride_y, stride_x, off_y0, off_x0, off_dy, off_dx, stream);
}

extern "C" int diga_conv2d_wgrad_bf16x6_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                              size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho,
                                              int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                              int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream) {
    DIGA_REQUIRE(dy_ld >= 0 && x_ld >= 0, DIGA_EINVAL, "conv2d_wgrad_bf16x6_f32in: dy_ld / x_ld must be at least the channel count");
    return conv2d_wgrad_bf16x6_impl(dy, dy_ld, x, x_ld, dw, workspace, workspace_bytes, N, Hi, Wi, Cin, Ho, Wo, Cout, R, S, stride_y,
                                    stride_x, off_y0, off_x0, off_dy, off_dx, stream);
}

// The weight gradient of a multi-tap convolution on the loader form: diga_conv2d_wgrad_bf16x6_f32in's arguments with
// 1 <= R * S <= 64, dw [Cout][R][S][Cin]; the split-K plan counts the taps (plan_wgrad_x6(M, Cout, Cin, R * S)).
extern "C" size_t diga_conv_taps_wgrad_bf16x6_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R,
                                                              int64_t S) {
    if (!taps_wgrad_shape_ok(N, Ho, Wo, Cout, Cin, R, S)) return 0;
    const int64_t M = N * Ho * Wo, RS = R * S;
    return wgrad_slab_bytes(plan_wgrad_x6(M, Cout, Cin, RS), Cout, Cin, RS) + (size_t)RS * wgrad_mpad(M) * sizeof(int) + 64;
}

extern "C" int diga_conv_taps_wgrad_bf16x6_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                                 size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho,
                                                 int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                                 int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream) {
    DIGA_REQUIRE(dy_ld >= 0 && x_ld >= 0, DIGA_EINVAL, "conv_taps_wgrad_bf16x6_f32in: dy_ld / x_ld must be at least the channel count");
    return conv2d_wgrad_bf16x6_impl(dy, dy_ld, x, x_ld, dw, workspace, workspace_bytes, N, Hi, Wi, Cin, Ho, Wo, Cout, R, S, stride_y,
                                    stride_x, off_y0, off_x0, off_dy, off_dx, stream, true);
}

// ---- the Winograd-domain GEMMs on bf16x6 (winograd.hip: diga_conv2d_winograd_bf16x6 / diga_conv2d_wgrad_winograd_bf16x6)
namespace diga {

// `batches` weight images, consecutive: image b = diga_split_bf16x6_image(U + b * Cout * K, ..., Cout, 1, K), one launch.
int split_image3_batched(const float* U, void* imgs, int batches, int64_t Cout, int64_t K, hipStream_t st) {
    const int64_t bn = image_bn(Cout);
    const int64_t total = ceil_div(Cout, bn) * (K / 32) * bn * 4;
    int64_t blocks = ceil_div(total, 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(split_image3_batched_kernel, dim3((unsigned)blocks, (unsigned)batches), dim3(256), 0, st, U, (unsigned char*)imgs,
                       (int)Cout, (int)K, (int)bn, total, Cout * K, (int64_t)diga_split_bf16x6_image_bytes(Cout, 1, K));
    return DIGA_OK;
}

// shape rules of gemm_batched_bf16x6 (shared by the entry points' checks and the workspace queries)
bool gemm_batched_bf16x6_ok(int64_t rows_per_batch, int64_t batches, int64_t K, int64_t Cout) {
    if (rows_per_batch <= 0 || rows_per_batch % 256 != 0 || batches <= 0 || batches >= 65536 || K <= 0 || K % 32 != 0 || Cout <= 64 ||
        Cout % 4 != 0)
        return false;
    const int64_t M = rows_per_batch * batches;
    return M < (1ll << 31) && (M / 256) * ceil_div(Cout, 128) < (1ll << 31);
}

// out_b [rows x Cout] = A_b [rows x K] * W_b^T for `batches` products stacked row-wise (A [batches * rows][K] fp32, read in place
// and split by the loader waves; out likewise; W_b as the b-th pre-split image of `imgs`) in one launch of
// conv_fwd_x6_kernel<2, false, true, true>.  The arguments must pass gemm_batched_bf16x6_ok.
int gemm_batched_bf16x6(const float* A, int64_t rows_per_batch, int batches, int64_t K, const void* imgs, int64_t Cout, float* out,
                        hipStream_t st) {
    DIGA_REQUIRE(gemm_batched_bf16x6_ok(rows_per_batch, batches, K, Cout), DIGA_EINVAL,
                 "gemm_batched_bf16x6: rows %% 256, K %% 32, Cout %% 4 (> 64) required; rows * batches and the tile count below 2^31");
    const int64_t M = rows_per_batch * batches;
    ConvArgs a;
    a.in = A; a.wgt = nullptr; a.wgt_hi = nullptr; a.wgt_lo = nullptr;
    a.wgt_img = reinterpret_cast<const unsigned char*>(imgs); a.bias = nullptr; a.out = out; a.stats = nullptr;
    a.N = 1; a.Hi = (int)(M / 256); a.Wi = 256; a.Cin = (int)K; a.in_ld = (int)K;
    a.Ho = a.Hi; a.Wo = 256; a.Cout = (int)Cout; a.out_ld = (int)Cout;
    a.R = 1; a.S = 1; a.sy = 1; a.sx = 1; a.oy0 = 0; a.ox0 = 0; a.ody = 1; a.odx = 1;
    a.M = (int)M;
    a.tiles_m = (int)(M / 256);
    a.tiles_n = (int)ceil_div(Cout, 128);
    a.all_inside = 1;
    set_options(a, nullptr);
    {
        const int rc = set_bwd_epilogue(a, nullptr, "gemm_batched_bf16x6");
        if (rc) return rc;
    }
    a.wb_tiles = (int)(rows_per_batch / 256);
    a.wb_stride = (int64_t)diga_split_bf16x6_image_bytes(Cout, 1, K);        // (bytes: the images are byte arrays)
    const size_t ring = (size_t)2 * (3 * 256 * 64 + 3 * 128 * 64);
    const size_t stg = (size_t)2 * 128 * (128 + 4) * sizeof(float);
    const size_t sh = ring > stg ? ring : stg;
    DIGA_LAUNCH_K((conv_fwd_x6_kernel<2, false, true, true>), 768, sh);
    return DIGA_OK;
}

bool wgrad_batched_bf16x6_ok(int64_t rows, int64_t batches, int64_t Cout, int64_t Cin) {
    if (rows <= 0 || rows % 32 != 0 || rows >= (1ll << 31) || batches <= 0 || batches >= 65536 || Cout <= 0 || Cout % 256 != 0 ||
        Cin <= 0 || Cin % 128 != 0)
        return false;
    const WgradPlan p = plan_wgrad_x6(rows, Cout, Cin, batches);
    return (int64_t)p.tiles_m * p.tiles_n * batches * p.splits < (1ll << 31);
}
size_t wgrad_batched_bf16x6_slab_bytes(int64_t rows, int batches, int64_t Cout, int64_t Cin) {
    return wgrad_slab_bytes(plan_wgrad_x6(rows, Cout, Cin, batches), Cout, Cin, batches);
}
// dU_b [Cout x Cin] = Z_b^T V_b (contraction over the rows) for `batches` products in one launch of
// conv_wgrad_x6_kernel<true, true>: Z [batches][rows][Cout], V [batches][rows][Cin] fp32, dU [Cout][batches][Cin]; split-K by
// plan_wgrad_x6 (at least 8 K-steps per block, about two rounds of blocks), partial sums in `slab`
// (wgrad_batched_bf16x6_slab_bytes), added in fixed order.  The arguments must pass wgrad_batched_bf16x6_ok.
int wgrad_batched_bf16x6(const float* Z, const float* V, float* dU, float* slab, int64_t rows, int batches, int64_t Cout, int64_t Cin,
                         hipStream_t st) {
    DIGA_REQUIRE(wgrad_batched_bf16x6_ok(rows, batches, Cout, Cin), DIGA_EINVAL,
                 "wgrad_batched_bf16x6: rows %% 32, Cout %% 256, Cin %% 128 required; rows and the block count below 2^31");
    const WgradPlan p = plan_wgrad_x6(rows, Cout, Cin, batches);
    WgradArgs a;
    a.dy = Z; a.x = V; a.slab = p.splits > 1 ? slab : dU;
    a.N = 1; a.Hi = 1; a.Wi = (int)rows; a.Cin = (int)Cin; a.x_ld = (int)Cin;
    a.Ho = 1; a.Wo = (int)rows; a.Cout = (int)Cout; a.dy_ld = (int)Cout;
    a.R = 1; a.S = batches; a.sy = 1; a.sx = 1; a.oy0 = 0; a.ox0 = 0; a.ody = 1; a.odx = 1;
    a.M = (int)rows; a.tiles_m = p.tiles_m; a.tiles_n = p.tiles_n; a.splits = p.splits; a.steps_per_split = p.steps_per_split;
    a.ptab = nullptr; a.zeros = nullptr; a.M_pad = (int)rows;
    a.dy_tap_stride = rows * Cout;
    a.x_tap_stride = rows * Cin;
    const unsigned grid = (unsigned)((int64_t)p.tiles_m * p.tiles_n * batches * p.splits);
    const size_t sh = (size_t)2 * (3 * kBK * 512 + 3 * kBK * 256);
    (void)hipFuncSetAttribute((const void*)conv_wgrad_x6_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    hipLaunchKernelGGL((conv_wgrad_x6_kernel<true, true>), dim3(grid), dim3(512), sh, st, a);
    if (p.splits > 1) {
        const int64_t n4 = Cout * batches * Cin / 4;
        hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0, st, (const float*)slab, dU, n4, p.splits);
    }
    return DIGA_OK;
}

}  // namespace diga

extern "C" int diga_gemm_batched_bf16x6_f32in(const float* A, int64_t rows_per_batch, int64_t batches, int64_t K, const void* wgt_imgs,
                                              int64_t Cout, float* out, void* stream) {
    DIGA_REQUIRE(A && wgt_imgs && out, DIGA_EINVAL, "gemm_batched_bf16x6_f32in: null pointer");
    DIGA_REQUIRE(gemm_batched_bf16x6_ok(rows_per_batch, batches, K, Cout), DIGA_EINVAL,
                 "gemm_batched_bf16x6_f32in: rows_per_batch %% 256, K %% 32, Cout %% 4 (> 64) required; rows_per_batch * batches and "
                 "the tile count below 2^31");
    DIGA_REQUIRE(aligned16(A) && aligned16(wgt_imgs) && aligned16(out), DIGA_EALIGN, "gemm_batched_bf16x6_f32in: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(DIGA_PROF_CONV_FWD, st, 2.0 * (double)(rows_per_batch * batches) * (double)Cout * (double)K);
    const int rc = gemm_batched_bf16x6(A, rows_per_batch, (int)batches, K, wgt_imgs, Cout, out, st);
    return rc ? rc : launch_status("diga_gemm_batched_bf16x6_f32in");
}

extern "C" size_t diga_wgrad_batched_bf16x6_workspace_bytes(int64_t rows, int64_t batches, int64_t Cout, int64_t Cin) {
    if (!wgrad_batched_bf16x6_ok(rows, batches, Cout, Cin)) return 0;
    return wgrad_batched_bf16x6_slab_bytes(rows, (int)batches, Cout, Cin) + 64;
}

extern "C" int diga_wgrad_batched_bf16x6_f32in(const float* Z, const float* V, float* dU, void* workspace, size_t workspace_bytes,
                                               int64_t rows, int64_t batches, int64_t Cout, int64_t Cin, void* stream) {
    DIGA_REQUIRE(Z && V && dU && workspace, DIGA_EINVAL, "wgrad_batched_bf16x6_f32in: null pointer");
    DIGA_REQUIRE(wgrad_batched_bf16x6_ok(rows, batches, Cout, Cin), DIGA_EINVAL,
                 "wgrad_batched_bf16x6_f32in: rows %% 32, Cout %% 256, Cin %% 128 required; rows and the block count below 2^31");
    DIGA_REQUIRE(aligned16(Z) && aligned16(V) && aligned16(dU) && aligned16(workspace), DIGA_EALIGN,
                 "wgrad_batched_bf16x6_f32in: pointers must be 16-byte aligned");
    DIGA_REQUIRE(workspace_bytes >= diga_wgrad_batched_bf16x6_workspace_bytes(rows, batches, Cout, Cin), DIGA_EWORKSPACE,
                 "wgrad_batched_bf16x6_f32in: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(DIGA_PROF_CONV_BWD_WEIGHT, st, 2.0 * (double)(rows * batches) * (double)Cout * (double)Cin);
    const int rc = wgrad_batched_bf16x6(Z, V, dU, (float*)workspace, rows, (int)batches, Cout, Cin, st);
    return rc ? rc : launch_status("diga_wgrad_batched_bf16x6_f32in");
}
