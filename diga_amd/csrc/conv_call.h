// Host side only: the call records behind the convolution entry points (conv.hip, conv_bf16x6.h, winograd.hip) and the one
// copy of each public descriptor's rules.  An `extern "C"` entry point fills a record by name, applies its own null-descriptor
// rule and calls its family's launcher; nothing below the entry points takes the geometry as a positional list.
#pragma once
#include "common.h"

namespace diga {

// input coordinate = out * stride + off0 + tap * off_d (include/diga_hip.h)
struct ConvGeometry {
    int64_t N = 0, Hi = 0, Wi = 0, Cin = 0, Ho = 0, Wo = 0, Cout = 0, R = 0, S = 0;
    int64_t stride_y = 0, stride_x = 0, off_y0 = 0, off_x0 = 0, off_dy = 0, off_dx = 0;
    void* stream = nullptr;
};

// The entry points name these parameters alike: copy them into a record (ConvCall / WgradCall) by name.
#define DIGA_FILL_GEOMETRY(c_)                                                                                          \
    do {                                                                                                               \
        (c_).N = N; (c_).Hi = Hi; (c_).Wi = Wi; (c_).Cin = Cin; (c_).Ho = Ho; (c_).Wo = Wo; (c_).Cout = Cout;           \
        (c_).R = R; (c_).S = S; (c_).stride_y = stride_y; (c_).stride_x = stride_x;                                     \
        (c_).off_y0 = off_y0; (c_).off_x0 = off_x0; (c_).off_dy = off_dy; (c_).off_dx = off_dx; (c_).stream = stream;   \
    } while (0)

// forward / backward-data convolution: every family reads the fields it knows and leaves the others at their defaults
struct ConvCall : ConvGeometry {
    const void* in = nullptr;          // the fp32 tensor (row pitch in_ld) or a pre-split twin / triplet image (in_ld < 0)
    int64_t in_ld = -1;
    const float* wgt = nullptr;        // fp32 weights, or
    const uint16_t* wgt_hi = nullptr;  // the two split-bf16 planes, or
    const uint16_t* wgt_lo = nullptr;
    const void* wgt_img = nullptr;     // a pre-split weight image
    const float* bias = nullptr;
    float* out = nullptr;
    int64_t out_ld = 0;
    float* stats = nullptr;
    int prof_tag = 0;
    const diga_bwd_epilogue_t* epi = nullptr;
    const diga_conv_options_t* opts = nullptr;
    const diga_infer_epilogue_t* infer = nullptr;
    bool f32in = false;                // bf16x6: the loader form (fp32 input, split in the loader waves)
    bool taps = false;                 // bf16x6: the multi-tap entry points (diga_conv_taps_*)
};

// weight gradient
struct WgradCall : ConvGeometry {
    const void* dy = nullptr;          // fp32 tensors (row pitches dy_ld / x_ld) or pre-split images (pitches < 0)
    const void* x = nullptr;
    int64_t dy_ld = -1, x_ld = -1;
    float* dw = nullptr;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    bool f32in = false, taps = false;  // as in ConvCall
    bool fit = false;                  // bf16x6: diga_wgrad_bf16x6_tiled_f32in (the tile by the tile rule, Cin % 8 for a single tap)
};

// kernel variant by epilogue: the index of the per-family kernel tables
enum ConvVariant { kPlain = 0, kEpi = 1, kInfer = 2 };
static inline ConvVariant conv_variant(const diga_bwd_epilogue_t* epi, const diga_infer_epilogue_t* infer) {
    return epi != nullptr ? kEpi : infer != nullptr ? kInfer : kPlain;
}

// The rules of diga_bwd_epilogue_t (nullptr = plain convolution: nothing to check).  out_ok: the caller's own demands on the
// output side (the direct kernels: Cout % 4, out_ld % 4, aligned output, no bias, no statistics), answered after the empty rule.
static int check_bwd_epilogue(const diga_bwd_epilogue_t* e, int64_t Cout, const char* who, bool out_ok = true) {
    if (e == nullptr) return DIGA_OK;
    DIGA_REQUIRE(e->addend || e->mask_y || e->mask_bits || e->x, DIGA_EINVAL, "%s: empty epilogue descriptor", who);
    DIGA_REQUIRE(out_ok, DIGA_EINVAL,
                 "%s: a backward epilogue needs Cout %% 4 == 0, out_ld %% 4 == 0, a 16-byte aligned output, no bias, no forward statistics", who);
    DIGA_REQUIRE(!e->addend || (aligned16(e->addend) && e->addend_ld >= Cout && e->addend_ld % 4 == 0), DIGA_EINVAL, "%s: bad addend", who);
    DIGA_REQUIRE(!e->mask_y || (aligned16(e->mask_y) && e->mask_ld >= Cout && e->mask_ld % 4 == 0), DIGA_EINVAL, "%s: bad mask_y", who);
    DIGA_REQUIRE(!e->x || (aligned16(e->x) && e->x_ld >= Cout && e->x_ld % 4 == 0), DIGA_EINVAL, "%s: bad x", who);
    DIGA_REQUIRE((e->mask_y != nullptr) + (e->relu_ab != nullptr) + (e->mask_bits != nullptr) <= 1, DIGA_EINVAL,
                 "%s: give one of mask_y, mask_bits, relu_ab", who);
    DIGA_REQUIRE(!e->mask_bits || e->mask_bits_ld * 8 >= Cout, DIGA_EINVAL, "%s: bad mask_bits", who);
    DIGA_REQUIRE(!e->relu_ab || (e->x && aligned16(e->relu_ab)), DIGA_EINVAL, "%s: relu_ab needs x", who);
    DIGA_REQUIRE(!e->partials || (e->x && e->mean && e->invstd && aligned16(e->mean) && aligned16(e->invstd)), DIGA_EINVAL,
                 "%s: partials need x, mean and invstd", who);
    return DIGA_OK;
}

// The rules of diga_infer_epilogue_t (nullptr: nothing to check).  out_ok: as above, answered after the coefficients' rule.
static int check_infer_epilogue(const diga_infer_epilogue_t* e, int64_t Cout, const float* out, const char* who, bool out_ok = true) {
    if (e == nullptr) return DIGA_OK;
    DIGA_REQUIRE(e->ab != nullptr && aligned16(e->ab), DIGA_EINVAL, "%s: the inference epilogue needs 16-byte aligned coefficients ab [2][Cout]", who);
    DIGA_REQUIRE(out_ok, DIGA_EINVAL,
                 "%s: the inference epilogue needs Cout %% 4 == 0, out_ld %% 4 == 0, 16-byte aligned pointers, no statistics", who);
    DIGA_REQUIRE(!e->residual || (aligned16(e->residual) && e->residual_ld >= Cout && e->residual_ld % 4 == 0 && e->residual != out),
                 DIGA_EINVAL, "%s: bad residual (16-byte aligned, residual_ld %% 4 == 0 and >= Cout, not the output)", who);
    return DIGA_OK;
}

// The multi-tap forms derive (Ho - 1) * stride + offset + (R - 1) * step in 32 bits: every term stays below 2^30.
// up_shift >= 0 (the `_opts` form: a checked diga_conv_options_t's upsample_shift): the coordinates are those of the upsampled image
// and map_tap mirrors them at 2 * (extent - 1), so the upsampled extents (Hi << up_shift, Wi << up_shift) stay below 2^30 as well.
static int check_tap_coordinates(const ConvGeometry& g, const char* who, int up_shift = -1) {
    const int64_t lim = 1ll << 30;
    DIGA_REQUIRE(up_shift < 0 || (g.Hi < lim && g.Wi < lim && (g.Hi << up_shift) < lim && (g.Wi << up_shift) < lim), DIGA_EINVAL,
                 "%s: the upsampled image lies beyond 32-bit pixel coordinates", who);
    DIGA_REQUIRE(g.stride_y < lim && g.stride_x < lim && g.off_y0 > -lim && g.off_y0 < lim && g.off_x0 > -lim && g.off_x0 < lim &&
                     g.off_dy > -lim && g.off_dy < lim && g.off_dx > -lim && g.off_dx < lim && g.Ho * g.stride_y < lim &&
                     g.Wo * g.stride_x < lim && (g.off_dy < 0 ? -g.off_dy : g.off_dy) * g.R < lim &&
                     (g.off_dx < 0 ? -g.off_dx : g.off_dx) * g.S < lim,
                 DIGA_EINVAL, "%s: strides / offsets beyond 32-bit pixel coordinates", who);
    return DIGA_OK;
}

}  // namespace diga
