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

// 8 consecutive fp32 channels (two float4) -> the three 16-byte plane words q0, q1, q2 (8 bf16 each, channel order).  Every kernel
// that makes planes -- the triplet pass, the weight images, the loader waves, the window fill -- makes them here: the same bits.
__device__ __forceinline__ void split3x8(const float4 lo, const float4 hi, uint4& q0, uint4& q1, uint4& q2) {
    uint2 a0, a1, a2, b0, b1, b2;
    split3x4(lo, a0, a1, a2);
    split3x4(hi, b0, b1, b2);
    q0 = make_uint4(a0.x, a0.y, b0.x, b0.y);
    q1 = make_uint4(a1.x, a1.y, b1.x, b1.y);
    q2 = make_uint4(a2.x, a2.y, b2.x, b2.y);
}

// THE product chain of bf16x6: per 16 x 16 sub-tile j and 32-deep K-step, a1 b1, a0 b2, a2 b0, a0 b1, a1 b0 chained from a ZERO
// accumulator (smallest first), a0 b0 into the running sum acc[j], then one fold add -- two roundings of the running sum per K-step.
// This order IS the bits of bf16x6 (tools/bf16x6_emulation.py restates it on the host); the forward, window and weight-gradient
// kernels differ in how the fragments reach the registers and in nothing here.  Each product runs over the NT column sub-tiles before
// the next starts, so an MFMA never waits for the one before it.
template <int NT>
__device__ __forceinline__ void x6_products(const bf16x8_t& a0, const bf16x8_t& a1, const bf16x8_t& a2, const bf16x8_t (&b0)[NT],
                                            const bf16x8_t (&b1)[NT], const bf16x8_t (&b2)[NT], f32x4 (&acc)[NT]) {
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
    for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[j], acc[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] += t[j];
}

// x [M][ld] fp32 (C channels) -> triplet [M][C/8][plane0 x 8 | plane1 x 8 | plane2 x 8]
__global__ __launch_bounds__(256) void make_triplet_kernel(const float* __restrict__ x, int64_t ld, unsigned char* __restrict__ trip,
                                                           int64_t M, int C8) {
    const int64_t total = M * C8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / C8;
        const int g = (int)(i - m * C8);
        const float* src = x + m * ld + g * 8;
        uint4* dst = reinterpret_cast<uint4*>(trip + i * 48);
        split3x8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), dst[0], dst[1], dst[2]);
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
        const int64_t plane = (int64_t)bn * 64;
        unsigned char* dst = img + tk * (3 * plane) + r * 64 + ((s ^ lds_swz(r)) << 4);
        split3x8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), *reinterpret_cast<uint4*>(dst),
                 *reinterpret_cast<uint4*>(dst + plane), *reinterpret_cast<uint4*>(dst + 2 * plane));
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
        const int64_t plane = (int64_t)bn * 64;
        unsigned char* dst = img + tk * (3 * plane) + r * 64 + ((s ^ lds_swz(r)) << 4);
        split3x8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), *reinterpret_cast<uint4*>(dst),
                 *reinterpret_cast<uint4*>(dst + plane), *reinterpret_cast<uint4*>(dst + 2 * plane));
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
// channels as two float4 (a wave instruction covers 16 rows x 128 contiguous bytes), splits them (split3x8) and writes the three
// planes with ds_write_b128 where the DMA form lands them.  The LDS image is byte-identical: MFMA waves, fold accumulator and
// drain_stage are shared.  Weights stay pre-split images staged by LDS-DMA.
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
// exact zeros.  It is the LS loader, written once: rows (x6_row), k-slot, swizzle, LDS slot, `issue`, `write` and the issue / vmcnt(0) /
// split / ds_write_b128 / lgkmcnt(0) / barrier ring are the same text; the pointwise form points its rows once and walks the chunks of
// its one tap, the tap walk derives (y0 + r * ody, x0 + q * odx) and the pointers per live tap (next_tap) -- null outside the image: no
// load is issued, the planes written are zero -- and steps K-step -> (tap, chunk).  R = S = 1 through the tap walk is the pointwise
// kernel's K-step sequence.  The MFMA waves learn the new K-step count and nothing else; drain_stage, the fold accumulator and the ring
// are untouched.
//
// OPT (diga_conv_taps_bf16x6_f32in_opts; TAPS, plain variant only): the input map of diga_conv_options_t folded into the tap walk.  A
// row's (y0, x0) are then coordinates in the LOGICAL image -- `in` upsampled by 2^up_shift, (Hi << up_shift) x (Wi << up_shift) -- and
// each tap's (y0 + r * ody, x0 + q * odx) goes through map_tap: mirrored at both borders under pad_reflect, clamped (so no geometry can
// form an address outside the tensor), shifted back to the source pixel; pix0 stays the SOURCE image's first pixel.  A tap that reads
// zero padding keeps the null pointer and the zero planes.  live_taps already counts in the logical extent and keeps every tap under
// pad_reflect; drain_stage already applies tanh under a.act.  An instantiation of its own: the others keep their instruction streams.
// Output row m of the tile (clamped to the last row) -> the first pixel of its image in `in` and the input coordinates of its tap (0, 0).
__device__ __forceinline__ void x6_row(const ConvArgs& a, int m, int& pix0, int& y0, int& x0) {
    m = min(m, a.M - 1);
    const int HoWo = a.Ho * a.Wo;
    const int img = m / HoWo, rem = m - img * HoWo;
    const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
    pix0 = img * a.Hi * a.Wi;
    y0 = ho * a.sy + a.oy0;
    x0 = wo * a.sx + a.ox0;
}

template <int TN, bool EPI = false, bool LS = false, bool WB = false, bool INF = false, bool TAPS = false, bool OPT = false>
__global__ __launch_bounds__(768, 3) void conv_fwd_x6_kernel(ConvArgs a) {
    static_assert(!(INF && (EPI || WB)), "the inference epilogue comes with the plain pointwise forward");
    static_assert(!TAPS || (LS && !WB), "the tap walk lives in the loader-split form");
    static_assert(!OPT || (TAPS && !EPI && !INF), "the folded input map comes with the plain multi-tap forward");
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

    if constexpr (LS) {
      if (loader) {
        const int lw = wv - 8;                                   // 0..3: A rows lw*64 + 16 j + (lane >> 2)
        const int lrow = lane >> 2;
        const int kslot = (lane & 3) ^ lds_swz(lrow);
        const int cchunks = a.Cin / 32;
        int pix0[4], y0[4], x0[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x6_row(a, m0 + lw * 64 + 16 * j + lrow, pix0[j], y0[j], x0[j]);
        const float* pa[4];
        auto point = [&](int dy, int dx) {                       // pa = the rows' pixels at tap offset (dy, dx); null outside the image
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iy = y0[j] + dy, ix = x0[j] + dx;
                if constexpr (OPT) {
                    int py, px;                                  // (always a pixel of the source image: map_tap clamps)
                    const bool ok = map_tap(a, iy, ix, py, px);
                    pa[j] = ok ? a.in + ((int64_t)pix0[j] + (int64_t)py * a.Wi + px) * a.in_ld + kslot * 8 : nullptr;
                } else {
                    const bool ok = (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
                    pa[j] = ok ? a.in + ((int64_t)pix0[j] + (int64_t)iy * a.Wi + ix) * a.in_ld + kslot * 8 : nullptr;
                }
            }
        };
        // the K-step in flight is chunk l_cc of tap l_tap.  Pointwise: one tap, whose chunks are the K-steps (l_cc = ks)
        [[maybe_unused]] uint64_t todo = live;
        [[maybe_unused]] int l_tap = 0, issued = 0;
        int l_cc = 0;
        auto next_tap = [&]() {                                  // -> l_tap = the next live tap, pa = its pixels
            l_tap = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int r = l_tap / a.S, q = l_tap - r * a.S;
            point(r * a.ody, q * a.odx);
        };
        const unsigned char* wimg = a.wgt_img;                   // the column tile's image: every tap's K-steps, live or not
        if constexpr (WB) wimg += (int64_t)(tile_m / a.wb_tiles) * a.wb_stride;
        const int64_t img_steps = TAPS ? (int64_t)a.R * a.S * cchunks : ksteps;
        const unsigned char* bimg = wimg + (int64_t)tile_n * img_steps * (3 * B_PLANE) + (lw * 3 * TN) * 1024 + lane * 16;
        float4 v[4][2];
        auto issue = [&](int buf) {                              // global loads of the next K-step into registers + its weight DMA
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pa[j] != nullptr) {
                    v[j][0] = *reinterpret_cast<const float4*>(pa[j] + l_cc * 32);
                    v[j][1] = *reinterpret_cast<const float4*>(pa[j] + l_cc * 32 + 4);
                }
            }
            const unsigned char* bsrc = bimg + (int64_t)(TAPS ? l_tap * cchunks + l_cc : l_cc) * (3 * B_PLANE);
            unsigned char* bdst = smem_b + buf * STAGE + 3 * A_PLANE + (lw * 3 * TN) * 1024;
#pragma unroll
            for (int c = 0; c < 3 * TN; ++c) DIGA_LDS_DMA16(bsrc + c * 1024, bdst + c * 1024);
        };
        auto write = [&](int buf) {                              // split + three ds_write_b128 per row, wait for them, step on
            unsigned char* stage = smem_b + buf * STAGE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;     // a pixel outside the image: zero planes
                if (pa[j] != nullptr) split3x8(v[j][0], v[j][1], q0, q1, q2);
                unsigned char* dst = stage + (lw * 64 + 16 * j) * 64 + lane * 16;
                *reinterpret_cast<uint4*>(dst) = q0;
                *reinterpret_cast<uint4*>(dst + A_PLANE) = q1;
                *reinterpret_cast<uint4*>(dst + 2 * A_PLANE) = q2;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            ++l_cc;
            if constexpr (TAPS) {
                ++issued;
                if (l_cc == cchunks) {                           // (pa changes only here, behind the writes that read it)
                    l_cc = 0;
                    if (issued < ksteps) next_tap();
                }
            }
        };
        if constexpr (TAPS) next_tap();
        else point(0, 0);
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
    } else if (loader) {
        const int lw = wv - 8;                                   // 0..3: A rows lw*64 + 16 j + (lane >> 2)
        const unsigned char* trip = reinterpret_cast<const unsigned char*>(a.in);
        const int lrow = lane >> 2;
        const int kslot = (lane & 3) ^ lds_swz(lrow);
        const int64_t rowb = (int64_t)a.Cin * 6;
        const unsigned char* pa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int pix0, iy, ix;
            x6_row(a, m0 + lw * 64 + 16 * j + lrow, pix0, iy, ix);
            const bool ok = (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
            pa[j] = ok ? trip + ((int64_t)pix0 + (int64_t)iy * a.Wi + ix) * rowb + kslot * 48 : nullptr;
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
            x6_products<NT>(a0, a1, a2, b0, b1, b2, acc[i]);
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
// backward-weight: conv_wgrad_x3t_kernel with a third plane, the product chain of x6_products and a two-stage ring.  One BM (Cout) x BN (Cin) tile per pixel range, tap and split: four MFMA waves as 2 x 2 (wave tile BM/2 x BN/2 =
// MT x NT sub-tiles of 16 x 16, MT = BM / 32, NT = BN / 32) + four loader waves; fragments through the transposing LDS reads; one
// x6_products per row of sub-tiles and 32-pixel K-step; the pixel clamp on dy; zero planes for x outside
// the image or past the pixel range; the channel-chunk clamp (kmax / cmax) with masked stores; the tap walk over a.ptab + tap *
// a.M_pad; the slab layout [split][Cout][RS][Cin].  Seven instantiations: 256 x 128 in the three forms below (238 of 256 VGPRs), and
// the loader form on 64 x 64, 64 x 128, 128 x 128, 256 x 64 for the layers that fill an eighth to a half of 256 x 128 and would pay
// six MFMAs per product on the padding (diga_wgrad_bf16x6_tiled_f32in).  A 16 x 16 sub-tile sees the same fragments and the same
// MFMA sequence on every tile: given the same pixel ranges a dw element has the same bits on any of them.
// ---------------------------------------------------------------------------------------------
//
// LS = false (the pass form, diga_conv2d_wgrad_bf16x6; 256 x 128 only): dy and x are triplet images, staged by LDS-DMA.
//
// LS (the `_f32in` entry points): dy and x are the fp32 tensors ([pixel][dy_ld] / [pixel][x_ld]); the loader lanes keep row,
// destination chunk, source-side swizzle and clamps, read their chunk's 8 channels as two float4, split (split3x8) and write the
// three planes into the lane-linear LDS slots of the DMA form -- the same LDS bytes, so the same dw bits.
// Loader split.  A plane is 32 pixel rows x CH / 8 chunks of 16 bytes (CH = BM or BN channels); the 256 loader lanes take
// 64 * 8 / CH rows per wave instruction, CH / 32 instructions per wave (4 / 2 / 1 at 256 / 128 / 64 channels): instruction j of wave
// wv covers rows 8 wv + (512 / CH) j + lane / (CH / 8), destination chunk lane % (CH / 8), and writes lane-linear (1 KB per plane
// and instruction).
//
// WB (wgrad_batched_bf16x6, the Winograd-domain weight gradient; loader form, 256 x 128 only): `R * S` independent products
// dU_b = Z_b^T V_b, the batch riding on the tap index as in conv_wgrad_dma_kernel -- tap b reads dy + b * a.dy_tap_stride and
// x + b * a.x_tap_stride (a.M rows each), the pixel table is the identity (a.ptab is null and not read), and a block's pixel range is
// clamped (dy) and zero-filled (x) within its batch's a.M rows.  The store is the un-batched one: slab [Cout][batches][Cin].
//
// Swizzle.  At CH >= 128 a pixel row is a whole number of 256-byte bank lines: chunk ^ (tr_key(r) << 1) moves the 32 bytes a lane
// group reads to one of 8 positions of the line.  At CH = 64 a row is 128 bytes: rows r and r + 1 share a bank line, so the row's
// parity already picks the half and the key has two bits,
//     key64(r) = ((r >> 1) & 1) | (((r >> 3) & 1) << 1),      chunk ^ (key64(r) << 1)   (bits 1..2 of the 3-bit chunk index).
// A transposing read serves 32 lanes at a time = the pixel rows {0..3, 8..11} (+ 4 for the second read, + 16 for the upper half), 32
// bytes of each.  The even rows of such a set (0, 2, 8, 10) lie on the low 128 bytes of their lines with the four keys 0, 1, 2, 3,
// the odd ones (1, 3, 9, 11) on the high 128 bytes with the same four: eight different 32-byte positions of the 256-byte line, all 64
// banks once, no conflict -- the property the wide key gives a 256-byte row.  The XOR touches bits below the row's chunk count only
// (0..6 of 8 chunks, 0..14 of 16 / 32), so every lane's address stays inside its own row and plane.  The MFMA waves never diverge:
// EXEC is full around every ds_read_tr16_b64.
//
// Residency (the ring is 2 x 3 x 32 x (BM + BN) x 2 bytes of the CU's 160 KB; a block is 8 waves, 2 per SIMD):
//     64 x 64: 48 KB, 3 blocks per CU (6 waves per SIMD: 80 VGPRs)        64 x 128: 72 KB, 2 blocks per CU (128 VGPRs)
//     128 x 128: 96 KB, 256 x 64: 120 KB and 256 x 128: 144 KB, 1 block per CU (no second ring fits) -- the first two win the padding only.
// wgrad_x6_tile_blocks is the one statement of that; __launch_bounds__, the dynamic LDS size and the split-K plan read it.
constexpr int wgrad_x6_tile_ring_bytes(int bm, int bn) { return 2 * 3 * kBK * (bm + bn) * 2; }
constexpr int wgrad_x6_tile_blocks(int bm, int bn) { return 160 * 1024 / wgrad_x6_tile_ring_bytes(bm, bn); }

template <int CH>
__device__ __forceinline__ int tile_key(int r) {
    if constexpr (CH >= 128) return tr_key(r) << 1;
    else return (((r >> 1) & 1) | (((r >> 3) & 1) << 1)) << 1;
}

template <int BM, int BN, bool LS = true, bool WB = false>
__global__ __launch_bounds__(512, 2 * wgrad_x6_tile_blocks(BM, BN)) void conv_wgrad_x6_kernel(WgradArgs a) {
    static_assert((BM == 64 || BM == 128 || BM == 256) && (BN == 64 || BN == 128), "tiles of 64 / 128 / 256 x 64 / 128 channels");
    static_assert(LS || (BM == 256 && BN == 128), "the LDS-DMA loader of the pass form is written for the 256 x 128 tile");
    static_assert(!WB || (LS && BM == 256 && BN == 128), "the batched form is the loader form on the 256 x 128 tile");
    constexpr int MT = BM / 32, NT = BN / 32;
    constexpr int A_ROW = BM * 2, B_ROW = BN * 2;                       // bytes per pixel row and plane
    constexpr int A_PLANE = kBK * A_ROW, B_PLANE = kBK * B_ROW, STAGE = 3 * A_PLANE + 3 * B_PLANE;
    static_assert(2 * STAGE == wgrad_x6_tile_ring_bytes(BM, BN), "the ring the launch asks for");
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
        constexpr int A_CPR = BM / 8, B_CPR = BN / 8;                   // 16-byte chunks per pixel row
        constexpr int A_RPI = 64 / A_CPR, B_RPI = 64 / B_CPR;           // pixel rows per wave instruction
        constexpr int A_NI = 8 / A_RPI, B_NI = 8 / B_RPI;               // instructions per loader wave and plane
        const int* tab = WB ? nullptr : a.ptab + (int64_t)tap * a.M_pad;
        // (a.dy / a.x are read where they are used, the table read is one conditional expression and the swizzle keys are derived at
        // their use: spelled so, every instantiation keeps the registers and the narrow tiles the instruction streams they had as
        // two templates -- profiles/r17_kernel_resources.md)
        const int64_t dy_tap = WB ? (int64_t)tap * a.dy_tap_stride : 0, x_tap = WB ? (int64_t)tap * a.x_tap_stride : 0;
        const int a_chunk_dst = lane & (A_CPR - 1), b_chunk_dst = lane & (B_CPR - 1);
        const int kgrp = k0 / 8, cgrp = c0 / 8, kmax = a.Cout / 8 - 1, cmax = a.Cin / 8 - 1;
        float4 va[A_NI][2], vb[B_NI][2];
        bool okb[B_NI];
        auto issue = [&](int ks) {                          // global loads of step ks into registers
#pragma unroll
            for (int j = 0; j < A_NI; ++j) {
                const int row = 8 * wv + A_RPI * j + lane / A_CPR;
                const int p = min(p_begin + ks * kBK + row, a.M - 1);
                const int chunk = min(kgrp + (a_chunk_dst ^ tile_key<BM>(row)), kmax);
                const float* src = a.dy + dy_tap + (int64_t)p * a.dy_ld + chunk * 8;
                va[j][0] = *reinterpret_cast<const float4*>(src);
                va[j][1] = *reinterpret_cast<const float4*>(src + 4);
            }
#pragma unroll
            for (int j = 0; j < B_NI; ++j) {
                const int row = 8 * wv + B_RPI * j + lane / B_CPR;
                const int p = p_begin + ks * kBK + row;
                int xi;                                     // (WB: the identity table)
                if constexpr (WB) xi = p < p_end ? p : -1;
                else xi = p < p_end ? tab[p] : -1;
                okb[j] = xi >= 0;
                if (okb[j]) {
                    const int chunk = min(cgrp + (b_chunk_dst ^ tile_key<BN>(row)), cmax);
                    const float* src = a.x + x_tap + (int64_t)xi * a.x_ld + chunk * 8;
                    vb[j][0] = *reinterpret_cast<const float4*>(src);
                    vb[j][1] = *reinterpret_cast<const float4*>(src + 4);
                }
            }
        };
        auto write = [&](int stg) {                         // split + ds_write_b128 of the three planes, then wait for them
            unsigned char* stage = smem_b + stg * STAGE;
#pragma unroll
            for (int j = 0; j < A_NI; ++j) {
                uint4 q0, q1, q2;
                split3x8(va[j][0], va[j][1], q0, q1, q2);
                unsigned char* dst = stage + (8 * wv + A_RPI * j) * A_ROW + lane * 16;
                *reinterpret_cast<uint4*>(dst) = q0;
                *reinterpret_cast<uint4*>(dst + A_PLANE) = q1;
                *reinterpret_cast<uint4*>(dst + 2 * A_PLANE) = q2;
            }
#pragma unroll
            for (int j = 0; j < B_NI; ++j) {
                uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;     // outside the image / past the pixel range: zero planes
                if (okb[j]) split3x8(vb[j][0], vb[j][1], q0, q1, q2);
                unsigned char* dst = stage + 3 * A_PLANE + (8 * wv + B_RPI * j) * B_ROW + lane * 16;
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
    auto a_off = [&](int tile, int row) { return row * A_ROW + (((2 * (wm * MT + tile) + (pp >> 1)) ^ tile_key<BM>(row)) << 4) + ((pp & 1) << 3); };
    auto b_off = [&](int tile, int row) { return row * B_ROW + (((2 * (wn * NT + tile) + (pp >> 1)) ^ tile_key<BN>(row)) << 4) + ((pp & 1) << 3); };

    __builtin_amdgcn_s_barrier();                          // stage 0 has landed
    for (int ks = 0; ks < ksteps; ++ks) {
        const unsigned char* Ap = smem_b + (ks & 1) * STAGE;
        const unsigned char* Bp = Ap + 3 * A_PLANE;
        bf16x8_t b0[NT], b1[NT], b2[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            b0[j] = tr_frag(Bp + b_off(j, row0), Bp + b_off(j, row1));
            b1[j] = tr_frag(Bp + B_PLANE + b_off(j, row0), Bp + B_PLANE + b_off(j, row1));
            b2[j] = tr_frag(Bp + 2 * B_PLANE + b_off(j, row0), Bp + 2 * B_PLANE + b_off(j, row1));
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const bf16x8_t a0 = tr_frag(Ap + a_off(i, row0), Ap + a_off(i, row1));
            const bf16x8_t a1 = tr_frag(Ap + A_PLANE + a_off(i, row0), Ap + A_PLANE + a_off(i, row1));
            const bf16x8_t a2 = tr_frag(Ap + 2 * A_PLANE + a_off(i, row0), Ap + 2 * A_PLANE + a_off(i, row1));
            x6_products<NT>(a0, a1, a2, b0, b1, b2, acc[i]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    float* out = a.slab + (int64_t)split * a.Cout * RS * a.Cin;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = c0 + wn * (BN / 2) + j * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = k0 + wm * (BM / 2) + i * 16 + (lane >> 4) * 4 + e;
                if (kk < a.Cout && c < a.Cin) out[((int64_t)kk * RS + tap) * a.Cin + c] = acc[i][j][e];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// "window form" of the multi-tap forward (diga_conv_window_bf16x6_f32in): stride 1 in the logical image (`in` after nearest upsampling,
// before padding), 2 <= R * S <= 64 taps.  conv_fwd_x6_kernel<..., TAPS> loads, splits and writes every input element once per tap; here a
// block owns kWinTH x kWinTW = 8 x 16 output pixels of ONE image (128 rows = 8 sub-tiles of 16 consecutive pixels of one output row) and
// splits that tile's input window -- WH x WW = (8 + (R - 1) dil_y) x (16 + (S - 1) dil_x) logical pixels of one 32-channel chunk --
// into LDS once; all R * S taps are then walked from LDS.  Loader work and L2 traffic per output fall by about the tap count.
//
// Window.  Pixel wp = wy * WW + wx of the window is the logical pixel (ho0 + oy0 + wy, wo0 + ox0 + wx); it goes through map_tap (mirror,
// clamp, shift back to the source pixel: no geometry forms an address outside the tensor; under up_shift neighbouring logical pixels
// repeat a source pixel and are stored once each, as logical pixels).  A pixel of the zero padding issues no load and gets zero planes.
// Per pixel and plane 64 bytes (32 channels), four 16-byte k-slots, slot s at s ^ lds_swz(wp); the three planes lie WH * WW * 64 bytes
// apart.  All four waves fill it: an item is (pixel, k-slot), read as two float4 at in_ld (a wave instruction covers 16 pixels x 128
// bytes), split3x8 and three ds_write_b128; four items are in flight per thread.
//
// K-steps.  One per (32-channel chunk, tap), CHUNK-major: one chunk's window is resident at a time, so the window costs
// WH * WW * 192 bytes whatever Cin is (7 x 7: 14 x 22 pixels = 57.8 KB; 5 x 5: 12 x 20 = 45 KB).  At Cin = 32 chunk-major and tap-major are
// the same sequence and a 16 x 16 sub-tile sees the fragments and the MFMA sequence of conv_fwd_x6_kernel<..., TAPS>: the same bits
// (taps that kernel steps over add exact zeros to a +0 start here).  At Cin > 32 the sums are reassociated across chunks.
// The A fragment of row (ty, tx) for tap (r, q) is window pixel (ty + r dil_y) * WW + tx + q dil_x = the row's own pixel + an offset that
// is uniform per K-step; lane l reads k-slot (l >> 4) ^ lds_swz(pixel) of it with ds_read_b128 -- the key is the same function of the
// window pixel index on both sides.  Bank behaviour: a ds_read_b128 is served in four groups of 16 lanes, 8 rows of one k-slot and 8 of
// the next; 16 consecutive pixels x 64 bytes span four 256-byte bank lines.  Enumerated on the host over every alignment of a
// sub-tile's first pixel (its own window pixel + the tap offset): where that index is a multiple of 8 the rows sit as in the M-tiled
// kernel and lds_swz spreads each group over all 16 slots of a line (no conflict); at every other alignment the key pattern is shifted
// against the lane groups and two lanes of a group meet on one slot (2-way, 8 instead of 4 LDS cycles per read), never more.  With six
// (16 columns) or 24 (64 columns) MFMAs behind three reads per sub-tile that stays under the MFMA time of the wide form and about
// level with it in the narrow one.  (Not measured with counters.)
//
// Weights.  The image of diga_split_bf16x6_image, unchanged; K-step (tap, chunk) sits at tap * Cin / 32 + chunk.  Two-stage ring by
// LDS-DMA, one barrier per K-step (it says "this step's weights have landed" and "the other stage is free").  NC = 64: the 64 rows of the
// column tile, 12 KB per K-step (column tile ct of a 128-row image = rows 64 (ct & 1) .. of image tile ct >> 1).  NC = 16 (Cout <= 16):
// rows 0 .. 15 of each plane only, 1 KB per plane and K-step; rows past Cout repeat the last channel and are never stored.  Cout > 64
// runs ceil(Cout / 64) column tiles, each of which loads and splits the window again.
//
// Products and drain.  x6_products per row of sub-tiles and K-step.  Plain drain only: the 128 x NC tile is staged over the (dead) window, then + bias, tanhf under a.act (drain_stage's expressions) and stores
// at out_ld masked by column and by the tile's ragged right / bottom edge.  No statistics, no epilogues.
//
// Residency.  LDS = ring (2 x 3 x NC x 64) + max(window, 128 x (NC + 4) x 4): 7 x 7 narrow 63.8 KB, 5 x 5 wide 69 KB -- two blocks of four
// waves per CU (2 waves per SIMD, 256 VGPRs each), so one block's window fill runs under the other's MFMAs.
//
// The three forms of the one kernel (the fill, the K-steps, the weight ring, the products and the drain are written once):
//   kWinAll   conv_win_x6_kernel<NC>: every tile of the output, as described above.
//   kWinRing  conv_win_x6_kernel<64, RING>: the same walk on the BORDER tiles only (by in {0, tiles_y - 1} or bx in {0, tiles_x - 1}; a block
//             index enumerates the top row, the bottom row, then the left / right tiles of the rows between).  Everything behind the block's
//             (img, by, bx, ct) is kWinAll's, so a ring tile's bits are the window form's.
//   kWinUp2   conv_up2_x6_kernel = conv_win_x6_kernel<64, false, UP2>: the INTERIOR tiles of a 2x nearest-upsampled input on phase-collapsed
//             weights (diga_conv_up2_bf16x6_f32in; the rule up2_x6_plan admits only calls whose interior taps all lie inside the logical
//             image; the ring form does the border tiles of the same call).  Output pixel (2 y + fy, 2 x + fx)
//             reads source rows y + a(fy, r), a(f, r) = floor((f + oy0 + r) / 2): per output phase (fy, fx) a stride-1 convolution of the SOURCE
//             image with R' x S' summed taps (diga_collapse_up2_weights) whose first tap sits at (a(fy, 0), a(fx, 0)).  A block does one phase
//             of 8 x 16 SOURCE pixels (grid anchored at the first interior output pixel = source pixel (4, 8)); its window is
//             (8 + R' - 1) x (16 + S' - 1) source pixels (5 x 5: 10 x 18 x 192 B = 34.6 KB), addresses clamped into the image (interior pixels
//             never read a clamped value under a non-zero weight); its weights are the phase's image, images image_bytes(Cout, R' S', Cin)
//             apart.  The launcher passes R', S' as a.R, a.S with unit dilation and leaves the call's own (oy0, ox0), Ho, Wo; stores are masked
//             to the pixels of interior tiles.  Per output pixel: the window form's K-step and product sequence on the collapsed weights.
constexpr int kWinTH = 8, kWinTW = 16;
constexpr int kWinAll = 0, kWinRing = 1, kWinUp2 = 2;

template <int NC, bool RING = false, bool UP2 = false>
__global__ __launch_bounds__(256, 2) void conv_win_x6_kernel(ConvArgs a) {
    constexpr int FORM = UP2 ? kWinUp2 : RING ? kWinRing : kWinAll;
    static_assert(!(RING && UP2), "a block is a ring tile or an interior tile");
    static_assert(NC == 16 || NC == 64, "16 output columns for Cout <= 16, 64 otherwise");
    static_assert(FORM == kWinAll || NC == 64, "the ring and the collapsed interior come with 64 columns");
    constexpr int NT = NC / 16, MT = 2, B_PLANE = NC * 64, WRING = 3 * B_PLANE, LDS_LD = NC + 4;
    extern __shared__ __align__(16) unsigned char smem_b[];
    unsigned char* const win = smem_b + 2 * WRING;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles_x = (a.Wo + kWinTW - 1) / kWinTW, tiles_y = (a.Ho + kWinTH - 1) / kWinTH;
    const int ct = wg % a.tiles_n;
    wg /= a.tiles_n;
    int bx, by, img, phy = 0, phx = 0;                           // (phy, phx): kWinUp2's output phase
    if constexpr (FORM == kWinUp2) {                             // (by, bx): a tile of SOURCE pixels, the four phases of one tile adjacent
        const int stx = (tiles_x - 1) >> 1, sty = (tiles_y - 1) >> 1;        // ceil(8 (tiles_x - 2) / 16), ceil(4 (tiles_y - 2) / 8)
        phx = wg & 1;
        phy = (wg >> 1) & 1;
        wg >>= 2;
        bx = wg % stx;
        wg /= stx;
        by = wg % sty;
        img = wg / sty;
    } else if constexpr (FORM == kWinRing) {
        const int ring = 2 * tiles_x + 2 * (tiles_y - 2);        // (tiles_x, tiles_y >= 3: the rule)
        const int i = wg % ring;
        img = wg / ring;
        if (i < 2 * tiles_x) {
            by = i < tiles_x ? 0 : tiles_y - 1;
            bx = i < tiles_x ? i : i - tiles_x;
        } else {
            by = 1 + ((i - 2 * tiles_x) >> 1);
            bx = (i & 1) ? tiles_x - 1 : 0;
        }
    } else {
        bx = wg % tiles_x;
        wg /= tiles_x;
        by = wg % tiles_y;
        img = wg / tiles_y;
    }
    // the tile's first output pixel; kWinUp2: its first SOURCE pixel, and the phase's first tap there
    const int ho0 = FORM == kWinUp2 ? 4 + by * kWinTH : by * kWinTH, wo0 = FORM == kWinUp2 ? 8 + bx * kWinTW : bx * kWinTW;
    const int ay0 = (phy + a.oy0) >> 1, ax0 = (phx + a.ox0) >> 1;            // floor((f + off0) / 2); read by kWinUp2 only
    const int WH = kWinTH + (a.R - 1) * a.ody, WW = kWinTW + (a.S - 1) * a.odx, WPLANE = WH * WW * 64;
    const int RS = a.R * a.S, cchunks = a.Cin / 32, ksteps = RS * cchunks;
    const int bn = a.Cout > 64 ? 128 : 64;                       // (image_bn: the weight image's tile)
    const int img_tile = NC == 16 ? 0 : (bn == 128 ? ct >> 1 : ct), img_half = (NC == 64 && bn == 128) ? (ct & 1) : 0;
    const unsigned char* wbase = a.wgt_img + (int64_t)img_tile * ksteps * (3 * bn * 64) + img_half * 4096 + lane * 16;
    if constexpr (FORM == kWinUp2) wbase += (int64_t)(phy * 2 + phx) * ((a.Cout + bn - 1) / bn) * ksteps * (3 * bn * 64);

    auto issue_w = [&](int tap, int cc, int buf) {               // LDS-DMA of K-step (tap, cc) into ring stage buf
        const unsigned char* src = wbase + (int64_t)(tap * cchunks + cc) * (3 * bn * 64);
        unsigned char* dst = smem_b + buf * WRING;
        if constexpr (NC == 16) {
            if (wv < 3) DIGA_LDS_DMA16(src + wv * (bn * 64), dst + wv * 1024);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int pc = wv * 3 + c;                       // plane pc >> 2, 1 KB piece pc & 3
                DIGA_LDS_DMA16(src + (pc >> 2) * (bn * 64) + (pc & 3) * 1024, dst + pc * 1024);
            }
        }
    };
    const int64_t pix0 = (int64_t)img * a.Hi * a.Wi;
    const int items = WH * WW * 4;
    auto load_window = [&](int cc) {                             // chunk cc of the tile's window: load, split, three planes
        for (int base = 0; base < items; base += 1024) {
            float4 v[4][2];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * 256 + t;
                const int wp = idx >> 2, wy = wp / WW, wx = wp - wy * WW;
                int py, px;                                      // (always a pixel of the source image: map_tap clamps)
                if constexpr (FORM == kWinUp2) {                 // a source pixel, clamped into the image
                    py = min(max(ho0 + ay0 + wy, 0), a.Hi - 1);
                    px = min(max(wo0 + ax0 + wx, 0), a.Wi - 1);
                    ok[u] = idx < items;
                } else {
                    ok[u] = map_tap(a, ho0 + a.oy0 + wy, wo0 + a.ox0 + wx, py, px) && idx < items;
                }
                if (ok[u]) {
                    const float* p = a.in + (pix0 + (int64_t)py * a.Wi + px) * a.in_ld + cc * 32 + (idx & 3) * 8;
                    v[u][0] = *reinterpret_cast<const float4*>(p);
                    v[u][1] = *reinterpret_cast<const float4*>(p + 4);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * 256 + t;
                if (idx < items) {
                    uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q2 = q0;     // zero padding: zero planes
                    if (ok[u]) split3x8(v[u][0], v[u][1], q0, q1, q2);
                    const int wp = idx >> 2;
                    unsigned char* dst = win + wp * 64 + (((idx & 3) ^ lds_swz(wp)) << 4);
                    *reinterpret_cast<uint4*>(dst) = q0;
                    *reinterpret_cast<uint4*>(dst + WPLANE) = q1;
                    *reinterpret_cast<uint4*>(dst + 2 * WPLANE) = q2;
                }
            }
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fk = lane >> 4;
    const int boff = frow * 64 + ((fk ^ lds_swz(frow)) << 4);
    int wp0[MT];                                                 // the rows' own window pixels: tile row wv * MT + i, column frow
#pragma unroll
    for (int i = 0; i < MT; ++i) wp0[i] = (wv * MT + i) * WW + frow;

    issue_w(0, 0, 0);
    int tap = 0, r = 0, q = 0, cc = 0;
    for (int ks = 0; ks < ksteps; ++ks) {
        if (tap == 0) {
            if (cc > 0) __syncthreads();                         // everyone has left the previous chunk's window
            load_window(cc);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();                                         // step ks's weights (and a new window) have landed; stage ks + 1 is free
        int ntap = tap + 1, ncc = cc;
        if (ntap == RS) {
            ntap = 0;
            ++ncc;
        }
        if (ks + 1 < ksteps) issue_w(ntap, ncc, (ks + 1) & 1);
        const unsigned char* B0 = smem_b + (ks & 1) * WRING + boff;
        bf16x8_t b0[NT], b1[NT], b2[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            b0[j] = *reinterpret_cast<const bf16x8_t*>(B0 + j * 1024);
            b1[j] = *reinterpret_cast<const bf16x8_t*>(B0 + B_PLANE + j * 1024);
            b2[j] = *reinterpret_cast<const bf16x8_t*>(B0 + 2 * B_PLANE + j * 1024);
        }
        const int toff = r * a.ody * WW + q * a.odx;             // uniform per K-step
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int wp = wp0[i] + toff;
            const unsigned char* A0 = win + wp * 64 + ((fk ^ lds_swz(wp)) << 4);
            const bf16x8_t a0 = *reinterpret_cast<const bf16x8_t*>(A0);
            const bf16x8_t a1 = *reinterpret_cast<const bf16x8_t*>(A0 + WPLANE);
            const bf16x8_t a2 = *reinterpret_cast<const bf16x8_t*>(A0 + 2 * WPLANE);
            x6_products<NT>(a0, a1, a2, b0, b1, b2, acc[i]);
        }
        if (++q == a.S) {
            q = 0;
            ++r;
        }
        if (++tap == RS) {
            tap = r = q = 0;
            ++cc;
        }
    }
    __syncthreads();                                             // everyone is out of the window: it becomes the drain's stage

    float* stage = reinterpret_cast<float*>(win);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) stage[((wv * MT + i) * 16 + fk * 4 + e) * LDS_LD + j * 16 + frow] = acc[i][j][e];
    __syncthreads();
    constexpr int CQ = NC / 4, RG = 256 / CQ;                    // column quads per row, rows per pass
    const int cq = t % CQ, rg = t / CQ;
    const int n = ct * NC + cq * 4;
    const bool vec_ok = (a.out_ld & 3) == 0 && n + 3 < a.Cout && ((uintptr_t)a.out & 15u) == 0;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias != nullptr) {
        bv.x = n + 0 < a.Cout ? a.bias[n + 0] : 0.f;
        bv.y = n + 1 < a.Cout ? a.bias[n + 1] : 0.f;
        bv.z = n + 2 < a.Cout ? a.bias[n + 2] : 0.f;
        bv.w = n + 3 < a.Cout ? a.bias[n + 3] : 0.f;
    }
#pragma unroll
    for (int p = rg; p < kWinTH * kWinTW; p += RG) {
        int ho = ho0 + (p >> 4), wo = wo0 + (p & 15);            // (kWinTW = 16)
        bool inside = ho < a.Ho && wo < a.Wo;
        if constexpr (FORM == kWinUp2) {                         // (ho, wo) is a source pixel: only pixels of interior tiles are this form's
            inside = ho < 4 * (tiles_y - 1) && wo < 8 * (tiles_x - 1);
            ho = 2 * ho + phy;
            wo = 2 * wo + phx;
        }
        if (inside && n < a.Cout) {
            float4 v = *reinterpret_cast<const float4*>(stage + p * LDS_LD + cq * 4);
            v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            if (a.act == 1) {
                v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w);
            }
            float* o = a.out + (((int64_t)img * a.Ho + ho) * a.Wo + wo) * a.out_ld + n;
            if (vec_ok) {
                store4_stream(o, v.x, v.y, v.z, v.w);
            } else {
                if (n + 0 < a.Cout) o[0] = v.x;
                if (n + 1 < a.Cout) o[1] = v.y;
                if (n + 2 < a.Cout) o[2] = v.z;
                if (n + 3 < a.Cout) o[3] = v.w;
            }
        }
    }
}

// (A body shared through a __device__ function gave the existing instantiations another register allocation; as one template they keep
// their instruction streams, and the collapsed interior is its third form under a name of its own.)
constexpr auto conv_up2_x6_kernel = conv_win_x6_kernel<64, false, true>;

// Phase-collapsed weights of a convolution on a 2x nearest-upsampled input: w [K][R][S][C] -> wc [fy][fx][K][RC][SC][C], element
// (r', s') = the sum of the taps (r, s) with a(fy, r) - a(fy, 0) == r' and a(fx, s) - a(fx, 0) == s', a(f, r) = floor((f + off0 + r) / 2):
// taken in double, in ascending (r, s) order, rounded to fp32 once (a phase with fewer taps keeps zeros in the rest).
__global__ __launch_bounds__(256) void collapse_up2_kernel(const float* __restrict__ w, float* __restrict__ wc, int K, int R, int S, int C,
                                                           int oy0, int ox0, int RC, int SC, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        int64_t u = i / C;
        const int sp = (int)(u % SC);
        u /= SC;
        const int rp = (int)(u % RC);
        u /= RC;
        const int k = (int)(u % K), ph = (int)(u / K);
        const int fy = ph >> 1, fx = ph & 1;
        const int ay0 = (fy + oy0) >> 1, ax0 = (fx + ox0) >> 1;
        double sum = 0.0;
        for (int r = 0; r < R; ++r) {
            if (((fy + oy0 + r) >> 1) - ay0 != rp) continue;
            for (int q = 0; q < S; ++q)
                if (((fx + ox0 + q) >> 1) - ax0 == sp) sum += (double)w[(((int64_t)k * R + r) * S + q) * C + c];
        }
        wc[i] = (float)sum;
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

// c.f32in: `in` is the fp32 tensor with row pitch in_ld (the loader form); else a triplet image (the pass form).
// c.infer: the inference epilogue (the `_infer` entry points; forward without statistics and without a backward epilogue), checked
// -- the rules of diga_conv2d_nhwc_f32_infer -- before anything is launched.
static int conv2d_bf16x6(const ConvCall& c) {
    DIGA_REQUIRE(c.in && c.wgt_img && c.out, DIGA_EINVAL, "conv2d_bf16x6: null pointer");
    DIGA_REQUIRE(c.N > 0 && c.Hi > 0 && c.Wi > 0 && c.Ho > 0 && c.Wo > 0 && c.Cout > 0, DIGA_EINVAL, "conv2d_bf16x6: bad shape");
    if (c.taps) {
        // the `diga_conv_taps_*` entry points (loader form only): up to 64 taps (live_taps' mask), every coordinate the loader
        // derives within 32 bits (check_tap_coordinates)
        DIGA_REQUIRE(c.in_ld >= 0, DIGA_EINVAL, "conv_taps_bf16x6: in_ld must be at least Cin and a multiple of 4");
        DIGA_REQUIRE(c.R >= 1 && c.S >= 1 && c.R <= 64 && c.S <= 64 && c.R * c.S <= 64, DIGA_EINVAL, "conv_taps_bf16x6: 1 <= R * S <= 64 taps");
        DIGA_REQUIRE(c.stride_y > 0 && c.stride_x > 0, DIGA_EINVAL, "conv_taps_bf16x6: strides must be positive");
        // c.opts (diga_conv_taps_bf16x6_f32in_opts): the plain forward only, and the tap coordinates are the upsampled image's
        DIGA_REQUIRE(!c.opts || (!c.stats && !c.epi && !c.infer), DIGA_EINVAL,
                     "conv_taps_bf16x6_opts: a folded input map / activation comes without statistics and without an epilogue");
        int rc = check_options(c.opts, "conv_taps_bf16x6_opts");
        if (rc) return rc;
        rc = check_tap_coordinates(c, "conv_taps_bf16x6", c.opts ? c.opts->upsample_shift : -1);
        if (rc) return rc;
    } else {
        DIGA_REQUIRE(c.R == 1 && c.S == 1 && c.stride_y > 0 && c.stride_x > 0, DIGA_EINVAL, "conv2d_bf16x6: pointwise (1x1) convolutions only");
    }
    DIGA_REQUIRE(c.Cin > 0 && c.Cin % 32 == 0 && c.out_ld >= c.Cout, DIGA_EINVAL, "conv2d_bf16x6: Cin must be a multiple of 32");
    DIGA_REQUIRE(!c.f32in || (c.in_ld >= c.Cin && c.in_ld % 4 == 0 && c.in_ld < (1ll << 31)), DIGA_EINVAL,
                 "conv2d_bf16x6_f32in: in_ld must be at least Cin and a multiple of 4");
    DIGA_REQUIRE(aligned16(c.in) && aligned16(c.wgt_img) && ((uintptr_t)c.out & 3u) == 0, DIGA_EALIGN, "conv2d_bf16x6: alignment");
    DIGA_REQUIRE(c.N * c.Hi * c.Wi < (1ll << 31) && c.N * c.Ho * c.Wo < (1ll << 31), DIGA_EINVAL, "conv2d_bf16x6: too many pixels");
    // every output pixel reads an input pixel inside the image or zeros: the loader checks the coordinate, so any
    // (stride, offset) is in bounds
    const int tn = c.Cout > 64 ? 2 : 1;                 // (= image_bn(Cout) / 64: the weight image's tile)
    const int64_t tiles_m = ceil_div(c.N * c.Ho * c.Wo, 256), tiles_n = ceil_div(c.Cout, 64 * tn);
    DIGA_REQUIRE(!c.taps || tiles_m * tiles_n < (1ll << 31), DIGA_EINVAL, "conv_taps_bf16x6: too many tiles for one launch");
    ConvArgs a;
    const int rc = fill_conv_args(a, c, "conv2d_bf16x6", "conv2d_bf16x6_infer");
    if (rc) return rc;
    a.tiles_m = (int)tiles_m;
    a.tiles_n = (int)tiles_n;
    DIGA_REQUIRE(!c.infer || (!c.epi && c.prof_tag != DIGA_PROF_CONV_BWD_DATA), DIGA_EINVAL,
                 "conv2d_bf16x6_infer: the inference epilogue comes with the forward (no backward epilogue)");
    hipStream_t st = (hipStream_t)c.stream;
    ProfScope prof(conv_prof_tag(c), st, conv_flops(c));
    // conv_fwd_x6_kernel<TN, EPI, F32IN, WB, INF, TAPS> by [form][tn - 1][variant]; the name launch_status reports by [form][infer]
    enum { kPass, kLoader, kTaps };
    static const ConvKernel kX6[3][2][3] = {
        {{conv_fwd_x6_kernel<1, false>, conv_fwd_x6_kernel<1, true>, conv_fwd_x6_kernel<1, false, false, false, true>},
         {conv_fwd_x6_kernel<2, false>, conv_fwd_x6_kernel<2, true>, conv_fwd_x6_kernel<2, false, false, false, true>}},
        {{conv_fwd_x6_kernel<1, false, true>, conv_fwd_x6_kernel<1, true, true>, conv_fwd_x6_kernel<1, false, true, false, true>},
         {conv_fwd_x6_kernel<2, false, true>, conv_fwd_x6_kernel<2, true, true>, conv_fwd_x6_kernel<2, false, true, false, true>}},
        {{conv_fwd_x6_kernel<1, false, true, false, false, true>, conv_fwd_x6_kernel<1, true, true, false, false, true>,
          conv_fwd_x6_kernel<1, false, true, false, true, true>},
         {conv_fwd_x6_kernel<2, false, true, false, false, true>, conv_fwd_x6_kernel<2, true, true, false, false, true>,
          conv_fwd_x6_kernel<2, false, true, false, true, true>}}};
    static const char* const kName[3][2] = {{"diga_conv2d_nhwc_bf16x6", "diga_infer_conv2d_nhwc_bf16x6"},
                                            {"diga_conv2d_nhwc_bf16x6_f32in", "diga_infer_conv2d_nhwc_bf16x6_f32in"},
                                            {"diga_conv_taps_bf16x6_f32in", "diga_infer_conv_taps_bf16x6_f32in"}};
    // ... and the multi-tap form with the folded input map (OPT; plain variant only) by [tn - 1]
    static const ConvKernel kX6Opt[2] = {conv_fwd_x6_kernel<1, false, true, false, false, true, true>,
                                         conv_fwd_x6_kernel<2, false, true, false, false, true, true>};
    const int form = c.taps ? kTaps : c.f32in ? kLoader : kPass;
    const size_t ring = (size_t)2 * (3 * 256 * 64 + 3 * 64 * tn * 64);
    const size_t stg = (size_t)2 * 128 * (64 * tn + 4) * sizeof(float);
    launch_k(c.opts ? kX6Opt[tn - 1] : kX6[form][tn - 1][conv_variant(c.epi, c.infer)], (unsigned)(a.tiles_m * a.tiles_n), 768,
             ring > stg ? ring : stg, st, a);
    return launch_status(c.opts ? "diga_conv_taps_bf16x6_f32in_opts" : kName[form][c.infer != nullptr]);
}

extern "C" int diga_conv2d_nhwc_bf16x6(const void* in_triplet, const void* wgt_img, const float* bias, float* out, int64_t N,
                                       int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                       int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                       int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag, void* stream) {
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in_triplet; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld; c.stats = stats_partial; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

extern "C" int diga_conv2d_nhwc_bf16x6_epi(const void* in_triplet, const void* wgt_img, float* out, int64_t N, int64_t Hi, int64_t Wi,
                                           int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                                           int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy,
                                           int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag, void* stream) {
    DIGA_REQUIRE(epi != nullptr, DIGA_EINVAL, "conv2d_bf16x6_epi: null epilogue descriptor");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in_triplet; c.wgt_img = wgt_img; c.out = out; c.out_ld = out_ld; c.epi = epi; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

extern "C" int diga_conv2d_nhwc_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out,
                                             int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                             int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                             int64_t off_x0, int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag,
                                             void* stream) {
    DIGA_REQUIRE(in_ld >= 0, DIGA_EINVAL, "conv2d_bf16x6_f32in: in_ld must be at least Cin and a multiple of 4");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = true; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld;
    c.stats = stats_partial; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

extern "C" int diga_conv2d_nhwc_bf16x6_f32in_epi(const float* in, int64_t in_ld, const void* wgt_img, float* out, int64_t N, int64_t Hi,
                                                 int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                                 int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                                 int64_t off_x0, int64_t off_dy, int64_t off_dx, const diga_bwd_epilogue_t* epi,
                                                 int prof_tag, void* stream) {
    DIGA_REQUIRE(epi != nullptr, DIGA_EINVAL, "conv2d_bf16x6_f32in_epi: null epilogue descriptor");
    DIGA_REQUIRE(in_ld >= 0, DIGA_EINVAL, "conv2d_bf16x6_f32in_epi: in_ld must be at least Cin and a multiple of 4");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = true; c.wgt_img = wgt_img; c.out = out; c.out_ld = out_ld; c.epi = epi; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

// The pointwise forward with the inference epilogue (include/diga_hip.h, diga_infer_epilogue_t): conv_fwd_x6_kernel<TN, ..., INF>.
extern "C" int diga_infer_conv2d_nhwc_bf16x6(const void* in_triplet, const void* wgt_img, const float* bias, float* out, int64_t N,
                                             int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                             int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                             int64_t off_dy, int64_t off_dx, const diga_infer_epilogue_t* infer, int prof_tag,
                                             void* stream) {
    DIGA_REQUIRE(infer != nullptr, DIGA_EINVAL, "conv2d_bf16x6_infer: null epilogue descriptor");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in_triplet; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld; c.infer = infer; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

extern "C" int diga_infer_conv2d_nhwc_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out,
                                                   int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                                   int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                                   int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                                   const diga_infer_epilogue_t* infer, int prof_tag, void* stream) {
    DIGA_REQUIRE(infer != nullptr, DIGA_EINVAL, "conv2d_bf16x6_f32in_infer: null epilogue descriptor");
    DIGA_REQUIRE(in_ld >= 0, DIGA_EINVAL, "conv2d_bf16x6_f32in_infer: in_ld must be at least Cin and a multiple of 4");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = true; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld; c.infer = infer;
    c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

// Multi-tap convolutions on the loader form (conv_fwd_x6_kernel<..., TAPS>): the argument lists of the pointwise `_f32in` entry
// points with 1 <= R * S <= 64; R = S = 1 gives the pointwise kernel's bits.
extern "C" int diga_conv_taps_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                           int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                           int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                           int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag, void* stream) {
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = c.taps = true; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld;
    c.stats = stats_partial; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

extern "C" int diga_conv_taps_bf16x6_f32in_epi(const float* in, int64_t in_ld, const void* wgt_img, float* out, int64_t N, int64_t Hi,
                                               int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R,
                                               int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                               int64_t off_dy, int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag,
                                               void* stream) {
    DIGA_REQUIRE(epi != nullptr, DIGA_EINVAL, "conv_taps_bf16x6_f32in_epi: null epilogue descriptor");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = c.taps = true; c.wgt_img = wgt_img; c.out = out; c.out_ld = out_ld; c.epi = epi;
    c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

extern "C" int diga_infer_conv_taps_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out,
                                                 int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                                 int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                                 int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                                 const diga_infer_epilogue_t* infer, int prof_tag, void* stream) {
    DIGA_REQUIRE(infer != nullptr, DIGA_EINVAL, "infer_conv_taps_bf16x6_f32in: null epilogue descriptor");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = c.taps = true; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld;
    c.infer = infer; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

// diga_conv_taps_bf16x6_f32in with the input map and the activation of diga_conv_options_t folded into the kernel
// (conv_fwd_x6_kernel<..., TAPS, OPT>): `in` is the SOURCE tensor [N][Hi][Wi], the offsets address its 2^upsample_shift upsampling,
// reflect_pad mirrors the taps outside it, activation 1 is tanh on the output.  Forward only: stats_partial must be null.
extern "C" int diga_conv_taps_bf16x6_f32in_opts(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out,
                                                int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                                int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                                int64_t off_x0, int64_t off_dy, int64_t off_dx, float* stats_partial,
                                                const diga_conv_options_t* opts, int prof_tag, void* stream) {
    DIGA_REQUIRE(opts != nullptr, DIGA_EINVAL, "conv_taps_bf16x6_opts: null options");
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = c.taps = true; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld;
    c.stats = stats_partial; c.opts = opts; c.prof_tag = prof_tag;
    return conv2d_bf16x6(c);
}

// ---- the window forms of the multi-tap forward (conv_win_x6_kernel): every tile from the layer's weights (diga_conv_window_bf16x6_f32in), or
// the interior of a 2x nearest-upsampled input on phase-collapsed weights inside a ring of border tiles (diga_conv_up2_bf16x6_f32in)
namespace {
// The LDS of a block whose window is wh x ww pixels of one 32-channel chunk: the weight ring + the larger of the window's three planes
// and the drain's staging of the 8 x 16 x cols tile.
inline int64_t x6_window_lds(int64_t wh, int64_t ww, int64_t cols) {
    const int64_t window = wh * ww * 3 * 64, stage = (int64_t)kWinTH * kWinTW * (cols + 4) * 4, ring = 2 * 3 * cols * 64;
    return ring + (window > stage ? window : stage);
}

// THE window rule (diga_conv_window_bf16x6_plan answers it; the entry point, its LDS size and the Python planner read nothing else):
// which calls the window form takes, on which tile and with how many output columns per block.  Stride 1 in the logical image is the
// entry point's signature.  The tile is 8 x 16 for every class; 16 columns serve Cout <= 16, 64 columns everything else; the window of
// one 32-channel chunk, the weight ring and the drain's staging must fit the CU's 160 KB.
struct X6Window {
    int th, tw, cols;
    int64_t lds;
};
bool window_x6_plan(int64_t Hi, int64_t Wi, int64_t Cin, int64_t Cout, int64_t R, int64_t S, int64_t dil_y, int64_t dil_x,
                    int64_t up_shift, X6Window& w) {
    if (Hi <= 0 || Wi <= 0 || Cin <= 0 || Cin % 32 != 0 || Cout <= 0) return false;
    if (R < 1 || S < 1 || R > 64 || S > 64 || R * S < 2 || R * S > 64) return false;
    if (dil_y < 1 || dil_x < 1 || dil_y > 4096 || dil_x > 4096 || up_shift < 0 || up_shift > 2) return false;
    w.th = kWinTH;
    w.tw = kWinTW;
    w.cols = Cout <= 16 ? 16 : 64;
    w.lds = x6_window_lds(kWinTH + (R - 1) * dil_y, kWinTW + (S - 1) * dil_x, w.cols);
    return w.lds <= 160 * 1024;
}

inline int64_t up2_a(int64_t phase, int64_t off0, int64_t r) {        // floor((phase + off0 + r) / 2): the source row of tap r
    const int64_t v = phase + off0 + r;
    return v >= 0 ? v / 2 : -((-v + 1) / 2);
}
inline int up2_taps(int64_t R, int64_t off0) {                        // R': the widest phase's collapsed tap count
    int64_t m = 0;
    for (int64_t f = 0; f < 2; ++f) m = std::max(m, up2_a(f, off0, R - 1) - up2_a(f, off0, 0) + 1);
    return (int)m;
}

// THE rule (diga_conv_up2_bf16x6_plan answers it; the entry point, its LDS size and the Python planner read nothing else): which window-form
// calls run their interior tiles on phase-collapsed weights.  The window rule must admit the call with 64 output columns; one level of
// upsampling, unit dilation, 2 .. 7 taps per axis, first tap at or before the pixel; an 8 x 16 tile grid with an interior (>= 3 x 3 tiles);
// and every tap of every pixel of the interior tiles -- rows [8, 8 (tiles_y - 1)), columns [16, 16 (tiles_x - 1)) -- inside the logical
// image [0, 2 Hi) x [0, 2 Wi): there the collapsed weights reproduce the layer, at the padding they cannot (logical -1 and -2 mirror to
// source rows 0 and 1; zero padding zeroes half a group), so the ring keeps the border tiles.
struct X6Up2 {
    int rc, sc;
    int64_t tiles_y, tiles_x, lds;
};
bool up2_x6_plan(int64_t Hi, int64_t Wi, int64_t Cin, int64_t Cout, int64_t Ho, int64_t Wo, int64_t R, int64_t S, int64_t off_y0,
                 int64_t off_x0, int64_t dil_y, int64_t dil_x, int64_t up_shift, int64_t reflect_pad, X6Up2& u) {
    X6Window w;
    if (!window_x6_plan(Hi, Wi, Cin, Cout, R, S, dil_y, dil_x, up_shift, w) || w.cols != 64) return false;
    if (up_shift != 1 || dil_y != 1 || dil_x != 1 || R < 2 || S < 2 || R > 7 || S > 7 || off_y0 > 0 || off_x0 > 0) return false;
    if (reflect_pad < 0 || reflect_pad > 1 || Ho <= 0 || Wo <= 0 || Hi >= (1ll << 29) || Wi >= (1ll << 29)) return false;
    u.tiles_y = ceil_div(Ho, (int64_t)kWinTH);
    u.tiles_x = ceil_div(Wo, (int64_t)kWinTW);
    if (u.tiles_y < 3 || u.tiles_x < 3) return false;
    if (kWinTH + off_y0 < 0 || kWinTH * (u.tiles_y - 1) - 1 + off_y0 + R - 1 > 2 * Hi - 1) return false;
    if (kWinTW + off_x0 < 0 || kWinTW * (u.tiles_x - 1) - 1 + off_x0 + S - 1 > 2 * Wi - 1) return false;
    u.rc = up2_taps(R, off_y0);
    u.sc = up2_taps(S, off_x0);
    u.lds = x6_window_lds(kWinTH + u.rc - 1, kWinTW + u.sc - 1, 64);
    return true;
}

// The argument rules of the two entry points, in the order they answer, each under the entry point's own name.  u == nullptr:
// diga_conv_window_bf16x6_f32in.  u != nullptr: diga_conv_up2_bf16x6_f32in -- the phases' images and the options are operands of their
// own, the tap count is the collapsed rule's to judge, and that rule (which holds the window rule) decides whether the call is taken.
// On success w (and *u) hold the plans.
struct X6WindowNames {
    const char *who, *form, *plan;
};
const X6WindowNames kX6WindowNames[2] = {{"conv_window_bf16x6", "window", "diga_conv_window_bf16x6_plan"},
                                         {"conv_up2_bf16x6", "collapsed", "diga_conv_up2_bf16x6_plan"}};
int check_window_call(const ConvCall& c, const void* wgt_img_phases, X6Window& w, X6Up2* u) {
    const X6WindowNames& n = kX6WindowNames[u != nullptr];
    DIGA_REQUIRE(c.in && c.wgt_img && c.out && (!u || (wgt_img_phases && c.opts)), DIGA_EINVAL, "%s: null pointer", n.who);
    DIGA_REQUIRE(c.N > 0 && c.Hi > 0 && c.Wi > 0 && c.Ho > 0 && c.Wo > 0 && c.Cout > 0, DIGA_EINVAL, "%s: bad shape", n.who);
    DIGA_REQUIRE(u || (c.R >= 1 && c.S >= 1 && c.R <= 64 && c.S <= 64 && c.R * c.S >= 2 && c.R * c.S <= 64), DIGA_EINVAL,
                 "%s: 2 <= R * S <= 64 taps", n.who);
    DIGA_REQUIRE(c.Cin > 0 && c.Cin % 32 == 0 && c.out_ld >= c.Cout, DIGA_EINVAL, "%s: Cin must be a multiple of 32", n.who);
    DIGA_REQUIRE(c.in_ld >= c.Cin && c.in_ld % 4 == 0 && c.in_ld < (1ll << 31) && c.out_ld < (1ll << 31), DIGA_EINVAL,
                 "%s: in_ld must be at least Cin and a multiple of 4", n.who);
    DIGA_REQUIRE(aligned16(c.in) && aligned16(c.wgt_img) && aligned16(wgt_img_phases) && ((uintptr_t)c.out & 3u) == 0 &&
                     ((uintptr_t)c.bias & 3u) == 0, DIGA_EALIGN, "%s: alignment", n.who);
    int rc = check_options(c.opts, n.who);
    if (rc) return rc;
    const int up = c.opts ? c.opts->upsample_shift : 0;
    rc = check_tap_coordinates(c, n.who, up);
    if (rc) return rc;
    DIGA_REQUIRE(window_x6_plan(c.Hi, c.Wi, c.Cin, c.Cout, c.R, c.S, c.off_dy, c.off_dx, up, w) &&
                     (!u || up2_x6_plan(c.Hi, c.Wi, c.Cin, c.Cout, c.Ho, c.Wo, c.R, c.S, c.off_y0, c.off_x0, c.off_dy, c.off_dx, up, c.opts->reflect_pad, *u)),
                 DIGA_EINVAL, "%s: the %s form does not take this call (%s)", n.who, n.form, n.plan);
    DIGA_REQUIRE(c.N * c.Hi * c.Wi < (1ll << 31) && c.N * c.Ho * c.Wo < (1ll << 31), DIGA_EINVAL, "%s: too many pixels", n.who);
    if (c.opts && c.opts->reflect_pad) {                          // a mirror reaches at most the far border (nn.ReflectionPad2d's rule)
        const int64_t Hl = c.Hi << up, Wl = c.Wi << up;
        const int64_t y_hi = c.Ho - 1 + c.off_y0 + (c.R - 1) * c.off_dy, x_hi = c.Wo - 1 + c.off_x0 + (c.S - 1) * c.off_dx;
        DIGA_REQUIRE(-c.off_y0 < Hl && -c.off_x0 < Wl && y_hi - (Hl - 1) < Hl && x_hi - (Wl - 1) < Wl, DIGA_EINVAL,
                     "%s: reflection padding must be smaller than the (upsampled) image", n.who);
    }
    return DIGA_OK;
}

int conv_window_bf16x6(const ConvCall& c) {
    X6Window w;
    int rc = check_window_call(c, nullptr, w, nullptr);
    if (rc) return rc;
    const int64_t tiles_n = ceil_div(c.Cout, w.cols);
    const int64_t grid = c.N * ceil_div(c.Ho, w.th) * ceil_div(c.Wo, w.tw) * tiles_n;
    DIGA_REQUIRE(grid < (1ll << 31), DIGA_EINVAL, "conv_window_bf16x6: too many tiles for one launch");
    ConvArgs a;
    rc = fill_conv_args(a, c, "conv_window_bf16x6", "conv_window_bf16x6");
    if (rc) return rc;
    a.tiles_n = (int)tiles_n;
    hipStream_t st = (hipStream_t)c.stream;
    ProfScope prof(conv_prof_tag(c), st, conv_flops(c));
    launch_k(w.cols == 16 ? conv_win_x6_kernel<16> : conv_win_x6_kernel<64>, (unsigned)grid, 256, (size_t)w.lds, st, a);
    return launch_status("diga_conv_window_bf16x6_f32in");
}

int conv_up2_bf16x6(const ConvCall& c, const void* wgt_img_phases) {
    X6Window w;
    X6Up2 u;
    int rc = check_window_call(c, wgt_img_phases, w, &u);
    if (rc) return rc;
    const int64_t tiles_n = ceil_div(c.Cout, (int64_t)64);
    // interior: one block per phase and 8 x 16 tile of the SOURCE pixels [4, 4 (tiles_y - 1)) x [8, 8 (tiles_x - 1)); ring: the border tiles
    const int64_t grid_in = c.N * ((u.tiles_y - 1) / 2) * ((u.tiles_x - 1) / 2) * 4 * tiles_n;
    const int64_t grid_ring = c.N * (u.tiles_x * u.tiles_y - (u.tiles_x - 2) * (u.tiles_y - 2)) * tiles_n;
    DIGA_REQUIRE(grid_in < (1ll << 31) && grid_ring < (1ll << 31), DIGA_EINVAL, "conv_up2_bf16x6: too many tiles for one launch");
    ConvArgs a;
    rc = fill_conv_args(a, c, "conv_up2_bf16x6", "conv_up2_bf16x6");
    if (rc) return rc;
    a.tiles_n = (int)tiles_n;
    ConvArgs in = a;                                             // the interior: R' x S' collapsed taps of the source image, the phases' images
    in.R = u.rc;
    in.S = u.sc;
    in.wgt_img = static_cast<const unsigned char*>(wgt_img_phases);
    hipStream_t st = (hipStream_t)c.stream;
    ProfScope prof(conv_prof_tag(c), st, conv_flops(c));
    launch_k(conv_up2_x6_kernel, (unsigned)grid_in, 256, (size_t)u.lds, st, in);
    launch_k(conv_win_x6_kernel<64, true>, (unsigned)grid_ring, 256, (size_t)w.lds, st, a);
    return launch_status("diga_conv_up2_bf16x6_f32in");
}
}  // namespace

// Returns 1 and the tile (th x tw output pixels, th * tw % 128 == 0) and the output columns per block (16 for Cout <= 16, else 64) where
// the window form takes a stride-1 convolution of R x S taps at dilation (dil_y, dil_x) on the 2^upsample_shift upsampling of an
// Hi x Wi x Cin image; 0 (and nothing written) where it does not.
extern "C" int diga_conv_window_bf16x6_plan(int64_t Hi, int64_t Wi, int64_t Cin, int64_t Cout, int64_t R, int64_t S, int64_t dil_y,
                                            int64_t dil_x, int64_t upsample_shift, int* th, int* tw, int* cols) {
    X6Window w;
    if (!th || !tw || !cols || !window_x6_plan(Hi, Wi, Cin, Cout, R, S, dil_y, dil_x, upsample_shift, w)) return 0;
    *th = w.th;
    *tw = w.tw;
    *cols = w.cols;
    return 1;
}

// The multi-tap forward on the window form: stride 1, taps at (off_y0 + r * dil_y, off_x0 + q * dil_x) of the logical image; `opts`
// (nullable) as in diga_conv_taps_bf16x6_f32in_opts.  Plain forward: bias, optional tanh, no statistics, no epilogue.
extern "C" int diga_conv_window_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                             int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                             int64_t R, int64_t S, int64_t off_y0, int64_t off_x0, int64_t dil_y, int64_t dil_x,
                                             const diga_conv_options_t* opts, int prof_tag, void* stream) {
    const int64_t stride_y = 1, stride_x = 1, off_dy = dil_y, off_dx = dil_x;
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = c.taps = true; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld;
    c.opts = opts; c.prof_tag = prof_tag;
    return conv_window_bf16x6(c);
}

// Returns 1 and the collapsed tap counts R' x S' where the window form of a convolution on the 2x nearest upsampling of an Hi x Wi x Cin
// image runs its interior tiles on phase-collapsed weights (diga_conv_up2_bf16x6_f32in); 0 (and nothing written) where it does not.
extern "C" int diga_conv_up2_bf16x6_plan(int64_t Hi, int64_t Wi, int64_t Cin, int64_t Cout, int64_t Ho, int64_t Wo, int64_t R, int64_t S,
                                         int64_t off_y0, int64_t off_x0, int64_t dil_y, int64_t dil_x, int64_t upsample_shift,
                                         int64_t reflect_pad, int* rc, int* sc) {
    X6Up2 u;
    if (!rc || !sc || !up2_x6_plan(Hi, Wi, Cin, Cout, Ho, Wo, R, S, off_y0, off_x0, dil_y, dil_x, upsample_shift, reflect_pad, u)) return 0;
    *rc = u.rc;
    *sc = u.sc;
    return 1;
}

// w_krsc [K][R][S][C] -> wc [phase_y][phase_x][K][R'][S'][C] (fp32; R' x S' as diga_conv_up2_bf16x6_plan reports them for these taps
// and offsets): each collapsed weight is the sum of its group of taps, taken in double in ascending (r, s) order and rounded once.
extern "C" int diga_collapse_up2_weights(const float* w_krsc, float* wc, int64_t K, int64_t R, int64_t S, int64_t C, int64_t off_y0,
                                         int64_t off_x0, void* stream) {
    DIGA_REQUIRE(w_krsc && wc && K > 0 && C > 0 && R >= 2 && S >= 2 && R <= 7 && S <= 7 && off_y0 <= 0 && off_x0 <= 0 &&
                     off_y0 > -(1ll << 30) && off_x0 > -(1ll << 30) && K * R * S * C < (1ll << 40), DIGA_EINVAL,
                 "collapse_up2_weights: 2 <= R, S <= 7 taps, offsets <= 0");
    DIGA_REQUIRE(aligned16(w_krsc) && aligned16(wc), DIGA_EALIGN, "collapse_up2_weights: pointers must be 16-byte aligned");
    const int rc = up2_taps(R, off_y0), sc = up2_taps(S, off_x0);
    const int64_t total = 4 * K * rc * sc * C;
    int64_t blocks = ceil_div(total, (int64_t)256);
    if (blocks > 8192) blocks = 8192;
    ProfScope prof(DIGA_PROF_ELEMENTWISE, (hipStream_t)stream, (double)K * R * S * C * 4.0);
    hipLaunchKernelGGL(collapse_up2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w_krsc, wc, (int)K, (int)R, (int)S,
                       (int)C, (int)off_y0, (int)off_x0, rc, sc, total);
    return launch_status("diga_collapse_up2_weights");
}

// The window form of a convolution on the 2x nearest upsampling of `in` with the interior on phase-collapsed weights: stride 1, unit
// dilation, taps at (off_y0 + r, off_x0 + q) of the logical image; opts non-null with upsample_shift = 1.  wgt_img: the layer's image
// (the ring of border tiles); wgt_img_phases: diga_split_bf16x6_image of the four [K][R'][S'][C] tensors of diga_collapse_up2_weights,
// consecutive (diga_split_bf16x6_image_bytes(Cout, R' * S', Cin) apart).  Two launches that write disjoint pixels.
extern "C" int diga_conv_up2_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const void* wgt_img_phases, const float* bias,
                                          float* out, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                                          int64_t out_ld, int64_t R, int64_t S, int64_t off_y0, int64_t off_x0,
                                          const diga_conv_options_t* opts, int prof_tag, void* stream) {
    const int64_t stride_y = 1, stride_x = 1, off_dy = 1, off_dx = 1;
    ConvCall c;
    DIGA_FILL_GEOMETRY(c);
    c.in = in; c.in_ld = in_ld; c.f32in = c.taps = true; c.wgt_img = wgt_img; c.bias = bias; c.out = out; c.out_ld = out_ld;
    c.opts = opts; c.prof_tag = prof_tag;
    return conv_up2_bf16x6(c, wgt_img_phases);
}

namespace {
// THE tile rule (diga_wgrad_bf16x6_tile answers it, nothing else decides): BM by Cout, BN by Cin; 128 x 64 is not instantiated
// (no layer of either network needs it) and answers 128 x 128.  Every entry point but diga_wgrad_bf16x6_tiled_f32in runs 256 x 128.
struct X6Tile {
    int bm, bn;
    bool wide() const { return bm == 256 && bn == 128; }
};
constexpr X6Tile kX6Wide = {256, 128};
X6Tile wgrad_x6_tile(int64_t Cout, int64_t Cin) {
    X6Tile t;
    t.bm = Cout <= 64 ? 64 : Cout <= 128 ? 128 : 256;
    t.bn = Cin <= 64 ? 64 : 128;
    if (t.bm == 128 && t.bn == 64) t.bn = 128;
    return t;
}
// The split-K plan: tiles counted at bm x bn, about two rounds of RESIDENT blocks -- 256 CUs x wgrad_x6_tile_blocks(bm, bn) of
// them: 512 on the 256 x 128 tile -- at least 8 K-steps (256 pixels) per block, at most 512 ranges:
//     splits = min( ceil(2 * 256 * blocks_per_cu / (tiles_m * tiles_n * RS)),  max(floor(ceil(M / 32) / 8), 1),  512 )
//     steps_per_split = ceil(ceil(M / 32) / splits),   splits = ceil(ceil(M / 32) / steps_per_split)
// Short pixel ranges are also what keeps the weight gradient's error at the exact-fp32 kernels' level: the running sum of a range is
// rounded twice per K-step, the slabs are then added in fixed order by slab_reduce_kernel.  (plan_wgrad_wide, tuned for the
// widest layers, leaves a narrow layer on ONE block walking every pixel: measured 5x the fp32 kernel's error on a 64 -> 64
// layer over 37 636 pixels.)  The cap binds where one or two tiles cover the layer (64 -> 64 1x1: 1536 wanted).  slab_reduce_kernel
// adds the ranges one after the other in 256-thread blocks of four dw elements per thread -- four blocks for a 64 x 64 dw -- so its
// time grows with the range count whatever the tile: measured on 64 -> 64 over 16 x 193 x 193 pixels, 1536 ranges 0.49 ms against
// the wide tile's 0.38 ms at 512.
// RS: independent products sharing the launch (taps; the batches of the Winograd-domain form; 1 for a pointwise layer).
WgradPlan plan_wgrad_x6(int64_t M, int64_t Cout, int64_t Cin, int64_t RS = 1, X6Tile t = kX6Wide) {
    WgradPlan p;
    p.tm = t.bm / 64;
    p.tn = t.bn / 64;
    p.tiles_m = (int)ceil_div(Cout, t.bm);
    p.tiles_n = (int)ceil_div(Cin, t.bn);
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n * RS, ksteps = ceil_div(M, kBK);
    int64_t splits = ceil_div((int64_t)2 * 256 * wgrad_x6_tile_blocks(t.bm, t.bn), tiles);
    const int64_t max_splits = ksteps / 8 > 0 ? ksteps / 8 : 1;
    if (splits > max_splits) splits = max_splits;
    if (splits > 512) splits = 512;
    p.steps_per_split = (int)ceil_div(ksteps, splits);
    p.splits = (int)ceil_div(ksteps, p.steps_per_split);
    return p;
}
// Shape rules of the loader-form weight gradients that take taps, on tile t (shared by the entry points' checks and their workspace
// queries).  fit: diga_wgrad_bf16x6_tiled_f32in, where Cin % 8 is enough for a single tap.
bool wgrad_x6_shape_ok(const ConvGeometry& g, X6Tile t, bool fit) {
    const int64_t lim = 1ll << 31;
    if (g.N <= 0 || g.Ho <= 0 || g.Wo <= 0 || g.R < 1 || g.S < 1 || g.R > 64 || g.S > 64 || g.R * g.S > 64 || g.Cin <= 0 ||
        g.Cin % (fit && g.R * g.S == 1 ? 8 : 32) != 0 || g.Cin >= lim || g.Cout <= 0 || g.Cout % 8 != 0 || g.Cout >= lim || g.N >= lim || g.Ho >= lim ||
        g.Wo >= lim || g.N * g.Ho >= lim || g.N * g.Ho * g.Wo >= lim)
        return false;
    const WgradPlan p = plan_wgrad_x6(g.N * g.Ho * g.Wo, g.Cout, g.Cin, g.R * g.S, t);
    return (int64_t)p.tiles_m * p.tiles_n * g.R * g.S * p.splits < lim;
}
// split-K slabs, the pixel table of all taps, 16 zero bytes
size_t wgrad_x6_workspace_bytes(const WgradPlan& p, int64_t M, int64_t Cout, int64_t Cin, int64_t RS) {
    return wgrad_slab_bytes(p, Cout, Cin, RS) + (size_t)RS * wgrad_mpad(M) * sizeof(int) + 64;
}
size_t wgrad_x6_workspace_query(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R, int64_t S, bool fit) {
    ConvGeometry g;
    g.N = N; g.Ho = Ho; g.Wo = Wo; g.Cout = Cout; g.Cin = Cin; g.R = R; g.S = S;
    const X6Tile t = fit ? wgrad_x6_tile(Cout, Cin) : kX6Wide;
    if (!wgrad_x6_shape_ok(g, t, fit)) return 0;
    const int64_t M = N * Ho * Wo, RS = R * S;
    return wgrad_x6_workspace_bytes(plan_wgrad_x6(M, Cout, Cin, RS, t), M, Cout, Cin, RS);
}
}  // namespace

// (the pointwise entry points' query checks no shape: its plan is the single-tap one)
extern "C" size_t diga_conv2d_wgrad_bf16x6_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin,
                                                           int64_t R, int64_t S) {
    return wgrad_x6_workspace_bytes(plan_wgrad_x6(N * Ho * Wo, Cout, Cin), N * Ho * Wo, Cout, Cin, R * S);
}

namespace {
// The words of one family of entry points: `who` in most messages, `ld` in the pitch rule's, `taps` in the tap-coordinate rule's
// (null: a pointwise family, which takes any offsets), `launch` for launch_status.
struct X6WgradNames {
    const char *who, *ld, *taps, *launch;
};
enum X6WgradFamily { kX6Pass, kX6Loader, kX6Taps, kX6Tiled };
const X6WgradNames kX6WgradNames[4] = {
    {"conv2d_wgrad_bf16x6", "conv2d_wgrad_bf16x6_f32in", nullptr, "diga_conv2d_wgrad_bf16x6"},
    {"conv2d_wgrad_bf16x6", "conv2d_wgrad_bf16x6_f32in", nullptr, "diga_conv2d_wgrad_bf16x6_f32in"},
    {"conv2d_wgrad_bf16x6", "conv2d_wgrad_bf16x6_f32in", "conv_taps_wgrad_bf16x6", "diga_conv_taps_wgrad_bf16x6_f32in"},
    {"wgrad_bf16x6_tiled_f32in", "wgrad_bf16x6_tiled_f32in", "wgrad_bf16x6_tiled_f32in", "diga_wgrad_bf16x6_tiled_f32in"}};
}  // namespace

// The one launcher of conv_wgrad_x6_kernel's un-batched forms, on tile t.  c.f32in: the operands are the fp32 tensors with row
// pitches dy_ld / x_ld (the loader form); else triplet images (the pass form).  c.taps: diga_conv_taps_wgrad_bf16x6_f32in, one block
// group per tap from the pixel table of all taps.  c.fit: diga_wgrad_bf16x6_tiled_f32in with t = wgrad_x6_tile's answer; every other
// entry point passes the 256 x 128 tile.  A tiled call whose tile is 256 x 128 continues, once its shape rule has passed, as the older
// entry point of its tap count: that family's checks, words and launch name.
static int conv2d_wgrad_bf16x6(const WgradCall& c, X6Tile t) {
    const X6WgradNames& entry = kX6WgradNames[c.fit ? kX6Tiled : c.taps ? kX6Taps : kX6Pass];
    DIGA_REQUIRE(c.dy && c.x && c.dw && c.workspace, DIGA_EINVAL, "%s: null pointer", entry.who);
    DIGA_REQUIRE(c.fit || (c.N > 0 && c.Hi > 0 && c.Wi > 0 && c.Ho > 0 && c.Wo > 0), DIGA_EINVAL, "conv2d_wgrad_bf16x6: bad shape");
    DIGA_REQUIRE(!entry.taps || (c.f32in && c.Hi > 0 && c.Wi > 0 && wgrad_x6_shape_ok(c, t, c.fit) && c.stride_y > 0 && c.stride_x > 0),
                 DIGA_EINVAL, "%s: 1 <= R * S <= 64, Cin %% 32%s, Cout %% 8, positive strides and a block count below 2^31 required",
                 entry.taps, c.fit ? " (% 8 for 1x1)" : "");
    const bool one_tap = c.R == 1 && c.S == 1;
    const X6WgradNames& n = kX6WgradNames[c.fit && !t.wide() ? kX6Tiled : c.taps || (c.fit && !one_tap) ? kX6Taps : c.f32in ? kX6Loader : kX6Pass];
    if (n.taps) {
        const int rc = check_tap_coordinates(c, n.taps);
        if (rc) return rc;
    } else {
        DIGA_REQUIRE(one_tap && c.stride_y > 0 && c.stride_x > 0, DIGA_EINVAL, "conv2d_wgrad_bf16x6: pointwise (1x1) convolutions only");
        DIGA_REQUIRE(c.Cin > 0 && c.Cin % 8 == 0 && c.Cout > 0 && c.Cout % 8 == 0, DIGA_EINVAL, "conv2d_wgrad_bf16x6: channel counts must be multiples of 8");
    }
    DIGA_REQUIRE(!c.f32in || (c.dy_ld >= c.Cout && c.dy_ld % 4 == 0 && c.x_ld >= c.Cin && c.x_ld % 4 == 0 && c.dy_ld < (1ll << 31) && c.x_ld < (1ll << 31)),
                 DIGA_EINVAL, "%s: dy_ld / x_ld must be at least the channel count and multiples of 4", n.ld);
    DIGA_REQUIRE(aligned16(c.dy) && aligned16(c.x) && aligned16(c.dw) && aligned16(c.workspace), DIGA_EALIGN, "%s: alignment", n.who);
    DIGA_REQUIRE(c.N * c.Hi * c.Wi < (1ll << 31) && c.N * c.Ho * c.Wo < (1ll << 31), DIGA_EINVAL, "%s: too many pixels", n.who);
    const int64_t RS = c.R * c.S, M = c.N * c.Ho * c.Wo, M_pad = wgrad_mpad(M);
    const WgradPlan p = plan_wgrad_x6(M, c.Cout, c.Cin, RS, t);
    DIGA_REQUIRE(c.workspace_bytes >= wgrad_x6_workspace_bytes(p, M, c.Cout, c.Cin, RS), DIGA_EWORKSPACE, "%s: workspace too small", n.who);
    WgradArgs a;
    fill_wgrad_args(a, c, p, M_pad);
    hipStream_t st = (hipStream_t)c.stream;
    ProfScope prof(DIGA_PROF_CONV_BWD_WEIGHT, st, 2.0 * (double)M * (double)c.Cout * (double)RS * (double)c.Cin);
    launch_pixtab(a, c, wgrad_slab_bytes(p, c.Cout, c.Cin, RS), st);
    // conv_wgrad_x6_kernel<BM, BN, LS> by [BM / 128][BN / 128][loader form]; the pass form exists on the 256 x 128 tile only
    static const WgradKernel kX6[3][2][2] = {
        {{nullptr, conv_wgrad_x6_kernel<64, 64>}, {nullptr, conv_wgrad_x6_kernel<64, 128>}},
        {{nullptr, nullptr}, {nullptr, conv_wgrad_x6_kernel<128, 128>}},
        {{nullptr, conv_wgrad_x6_kernel<256, 64>}, {conv_wgrad_x6_kernel<256, 128, false>, conv_wgrad_x6_kernel<256, 128, true>}}};
    launch_k(kX6[t.bm / 128][t.bn / 128][c.f32in], wgrad_grid(a), 512, (size_t)wgrad_x6_tile_ring_bytes(t.bm, t.bn), st, a);
    launch_slab_reduce(a, static_cast<const float*>(c.workspace), c.dw, st);
    return launch_status(n.launch);
}

extern "C" int diga_conv2d_wgrad_bf16x6(const void* dy_triplet, const void* x_triplet, float* dw, void* workspace,
                                        size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho,
                                        int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                        int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream) {
    WgradCall c;
    DIGA_FILL_GEOMETRY(c);
    c.dy = dy_triplet; c.x = x_triplet; c.dw = dw; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return conv2d_wgrad_bf16x6(c, kX6Wide);
}

extern "C" int diga_conv2d_wgrad_bf16x6_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                              size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho,
                                              int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                              int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream) {
    DIGA_REQUIRE(dy_ld >= 0 && x_ld >= 0, DIGA_EINVAL, "conv2d_wgrad_bf16x6_f32in: dy_ld / x_ld must be at least the channel count");
    WgradCall c;
    DIGA_FILL_GEOMETRY(c);
    c.dy = dy; c.dy_ld = dy_ld; c.x = x; c.x_ld = x_ld; c.f32in = true; c.dw = dw; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return conv2d_wgrad_bf16x6(c, kX6Wide);
}

// The weight gradient of a multi-tap convolution on the loader form: diga_conv2d_wgrad_bf16x6_f32in's arguments with
// 1 <= R * S <= 64, dw [Cout][R][S][Cin]; the split-K plan counts the taps (plan_wgrad_x6(M, Cout, Cin, R * S)).
extern "C" size_t diga_conv_taps_wgrad_bf16x6_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R,
                                                              int64_t S) {
    return wgrad_x6_workspace_query(N, Ho, Wo, Cout, Cin, R, S, false);
}

extern "C" int diga_conv_taps_wgrad_bf16x6_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                                 size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho,
                                                 int64_t Wo, int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x,
                                                 int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream) {
    DIGA_REQUIRE(dy_ld >= 0 && x_ld >= 0, DIGA_EINVAL, "conv_taps_wgrad_bf16x6_f32in: dy_ld / x_ld must be at least the channel count");
    WgradCall c;
    DIGA_FILL_GEOMETRY(c);
    c.dy = dy; c.dy_ld = dy_ld; c.x = x; c.x_ld = x_ld; c.f32in = c.taps = true; c.dw = dw; c.workspace = workspace;
    c.workspace_bytes = workspace_bytes;
    return conv2d_wgrad_bf16x6(c, kX6Wide);
}

// ---- the loader-form weight gradient on the tile that fits the layer
extern "C" int diga_wgrad_bf16x6_tile(int64_t Cout, int64_t Cin, int* bm, int* bn) {
    DIGA_REQUIRE(bm && bn, DIGA_EINVAL, "wgrad_bf16x6_tile: null pointer");
    DIGA_REQUIRE(Cout > 0 && Cout % 8 == 0 && Cin > 0 && Cin % 8 == 0, DIGA_EINVAL, "wgrad_bf16x6_tile: channel counts must be positive multiples of 8");
    const X6Tile t = wgrad_x6_tile(Cout, Cin);
    *bm = t.bm;
    *bn = t.bn;
    return DIGA_OK;
}

extern "C" size_t diga_wgrad_bf16x6_tiled_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R, int64_t S) {
    return wgrad_x6_workspace_query(N, Ho, Wo, Cout, Cin, R, S, true);
}

// The weight gradient of a pointwise or multi-tap convolution on the loader form, on the tile wgrad_x6_tile picks for the layer:
// the arguments of diga_conv_taps_wgrad_bf16x6_f32in.  A 256 x 128 shape runs what the existing entry points run.
extern "C" int diga_wgrad_bf16x6_tiled_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                             size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo,
                                             int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                             int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream) {
    DIGA_REQUIRE(dy_ld >= 0 && x_ld >= 0, DIGA_EINVAL, "wgrad_bf16x6_tiled_f32in: dy_ld / x_ld must be at least the channel count");
    WgradCall c;
    DIGA_FILL_GEOMETRY(c);
    c.dy = dy; c.dy_ld = dy_ld; c.x = x; c.x_ld = x_ld; c.f32in = c.fit = true; c.dw = dw; c.workspace = workspace;
    c.workspace_bytes = workspace_bytes;
    return conv2d_wgrad_bf16x6(c, wgrad_x6_tile(Cout, Cin));
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
    ConvCall c;                                            // the stacked rows as an M / 256 x 256 image under a 1x1 convolution
    c.in = A; c.in_ld = K; c.wgt_img = imgs; c.out = out; c.out_ld = Cout;
    c.N = 1; c.Hi = c.Ho = M / 256; c.Wi = c.Wo = 256; c.Cin = K; c.Cout = Cout;
    c.R = c.S = c.stride_y = c.stride_x = c.off_dy = c.off_dx = 1;
    ConvArgs a;
    (void)fill_conv_args(a, c, "gemm_batched_bf16x6", "gemm_batched_bf16x6");
    a.tiles_m = (int)(M / 256);
    a.tiles_n = (int)ceil_div(Cout, 128);
    a.all_inside = 1;
    a.wb_tiles = (int)(rows_per_batch / 256);
    a.wb_stride = (int64_t)diga_split_bf16x6_image_bytes(Cout, 1, K);        // (bytes: the images are byte arrays)
    const size_t ring = (size_t)2 * (3 * 256 * 64 + 3 * 128 * 64);
    const size_t stg = (size_t)2 * 128 * (128 + 4) * sizeof(float);
    launch_k<ConvArgs>(conv_fwd_x6_kernel<2, false, true, true>, (unsigned)(a.tiles_m * a.tiles_n), 768, ring > stg ? ring : stg, st, a);
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
// conv_wgrad_x6_kernel<256, 128, true, true>: Z [batches][rows][Cout], V [batches][rows][Cin] fp32, dU [Cout][batches][Cin]; split-K by
// plan_wgrad_x6 (at least 8 K-steps per block, about two rounds of blocks), partial sums in `slab`
// (wgrad_batched_bf16x6_slab_bytes), added in fixed order.  The arguments must pass wgrad_batched_bf16x6_ok.
int wgrad_batched_bf16x6(const float* Z, const float* V, float* dU, float* slab, int64_t rows, int batches, int64_t Cout, int64_t Cin,
                         hipStream_t st) {
    DIGA_REQUIRE(wgrad_batched_bf16x6_ok(rows, batches, Cout, Cin), DIGA_EINVAL,
                 "wgrad_batched_bf16x6: rows %% 32, Cout %% 256, Cin %% 128 required; rows and the block count below 2^31");
    WgradArgs a;
    fill_wgrad_batched(a, Z, V, dU, slab, rows, batches, Cout, Cin, plan_wgrad_x6(rows, Cout, Cin, batches));
    launch_k<WgradArgs>(conv_wgrad_x6_kernel<256, 128, true, true>, wgrad_grid(a), 512, (size_t)wgrad_x6_tile_ring_bytes(256, 128), st, a);
    launch_slab_reduce(a, slab, dU, st);
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
