// Device helpers of the planar YUV 4:2:0 decode, shared by yuv.hip (atmvfi_yuv420_to_rgb) and yuv_window.hip (atmvfi_yuv420_window):
// the source frame's description, sample and chroma-segment loads, the chroma filter, the matrix, q / 255 and one whole pixel.  The
// definition they implement is spelled out at the top of yuv.hip and in include/atmvfi.h; both files hold it to the same bits because
// they run the same functions.
#pragma once
#include "common.h"

namespace {

struct alignas(4) U32x2 {
    unsigned a, b;
};
struct alignas(4) U32x3 {
    unsigned a, b, c;
};
struct alignas(2) U16x1 {
    unsigned short v;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// rint(c * 2^14) of the float64 matrices of (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722), limited range scaled by 219 / 224
// (yuv.py derives them again; tests/test_yuv_cpu.py holds both to the table of the README)
struct Coeffs {
    int dec[5];         // kY, kRV, kGU, kGV, kBU
    int enc[3][3];      // rows Y, U, V over (R, G, B)
};
const Coeffs kCoeffs[2][2] = {      // [matrix][full_range]
    {{{19077, 26149, -6419, -13320, 33050}, {{4207, 8260, 1604}, {-2428, -4768, 7196}, {7196, -6026, -1170}}},
     {{16384, 22970, -5638, -11700, 29032}, {{4899, 9617, 1868}, {-2765, -5427, 8192}, {8192, -6860, -1332}}}},
    {{{19077, 29372, -3494, -8731, 34610}, {{2991, 10064, 1016}, {-1649, -5547, 7196}, {7196, -6536, -660}}},
     {{16384, 25802, -3069, -7670, 30402}, {{3483, 11718, 1183}, {-1877, -6315, 8192}, {8192, -7441, -751}}}},
};

// the resident frame and the constants of its format: the first members of every decode kernel's arguments
struct YuvSrc {
    const unsigned char* yuv;
    int H, W, ch, cw;
    long long uoff, voff;       // first U / V sample, in samples
    int kY, kRV, kGU, kGV, kBU, yo, mid, T;
};

inline YuvSrc make_src(const void* yuv, int H, int W, int depth, int matrix, int full_range) {
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    const Coeffs& c = kCoeffs[matrix][full_range];
    return YuvSrc{(const unsigned char*)yuv, H, W, ch, cw, (long long)H * W, (long long)H * W + (long long)ch * cw,
                  c.dec[0], c.dec[1], c.dec[2], c.dec[3], c.dec[4], depth == 10 ? 64 : (full_range ? 0 : 16), depth == 10 ? 512 : 128,
                  depth == 10 ? 16 : 14};
}

template <int DEPTH, bool AL>
__device__ __forceinline__ int sample(const unsigned char* p, long long i) {
    if (DEPTH == 8) return p[i];
    if (AL) return reinterpret_cast<const unsigned short*>(p)[i];
    return (int)p[2 * i] | ((int)p[2 * i + 1] << 8);
}

// seg[k] = plane[r][clamp(q - 1 + k, 0, cw - 1)], k = 0..3: every chroma column that luma columns 2q .. 2q + 3 touch
template <int DEPTH, bool AL>
__device__ __forceinline__ void load_seg(const YuvSrc& a, long long plane, int r, int q, int seg[4]) {
    const long long row = plane + (long long)r * a.cw;
    if (AL) {       // q even and cw even: (q, q + 1) is a naturally aligned pair inside the row
        seg[0] = sample<DEPTH, true>(a.yuv, row + max(q - 1, 0));
        if (DEPTH == 8) {
            const unsigned v = reinterpret_cast<const U16x1*>(a.yuv + row + q)->v;
            seg[1] = (int)(v & 0xffu);
            seg[2] = (int)(v >> 8);
        } else {
            const unsigned v = *reinterpret_cast<const unsigned*>(a.yuv + 2 * (row + q));
            seg[1] = (int)(v & 0xffffu);
            seg[2] = (int)(v >> 16);
        }
        seg[3] = sample<DEPTH, true>(a.yuv, row + min(q + 2, a.cw - 1));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) seg[k] = sample<DEPTH, false>(a.yuv, row + clampi(q - 1 + k, 0, a.cw - 1));
    }
}

// q / 255 for an integer q in 0..255 with the bits of the fp32 division (what frame_u8_to_f32 computes): q * r with r = fl(1 / 255), then
// one correction step in fused multiply-adds -- e = fl(q - 255 y), y + e r.  Equal to the division for all 256 values
// (tests/test_yuv_cpu.py checks every one in exact rational arithmetic); four instructions where the division's expansion takes ten, and
// this kernel is bound by its instruction count, not by HBM, while it divides (tools/bench_yuv.py).
__device__ __forceinline__ float q255(int q) {
    const float f = (float)q, r = 0x1.010102p-8f;
    const float y = f * r;
    return __fmaf_rn(__fmaf_rn(-255.0f, y, f), r, y);
}

__device__ __forceinline__ int chroma_mix(int c00, int c01, int c10, int c11, int wx0, int wx1) {
    return (3 * (wx0 * c00 + wx1 * c01) + (wx0 * c10 + wx1 * c11) + 8) >> 4;
}

// (__mul24: the full-rate 24-bit multiply; coefficients are below 2^17 and samples below 2^16, so the low 32 bits are the product's)
__device__ __forceinline__ void to_rgb(const YuvSrc& a, int Y, int U, int V, int q[3]) {
    const int y = __mul24(a.kY, Y - a.yo), u = U - a.mid, v = V - a.mid, half = 1 << (a.T - 1);
    q[0] = clip8((y + __mul24(a.kRV, v) + half) >> a.T);
    q[1] = clip8((y + __mul24(a.kGU, u) + __mul24(a.kGV, v) + half) >> a.T);
    q[2] = clip8((y + __mul24(a.kBU, u) + half) >> a.T);
}

// one frame pixel, every sample loaded on its own (the general path)
template <int DEPTH, bool LEFT>
__device__ __forceinline__ void decode_pixel(const YuvSrc& a, int fy, int fx, int q[3]) {
    const int r0 = fy >> 1, r1 = clampi(r0 + ((fy & 1) ? 1 : -1), 0, a.ch - 1);
    const int q0 = fx >> 1;
    const int q1 = LEFT ? min(q0 + 1, a.cw - 1) : clampi(q0 + ((fx & 1) ? 1 : -1), 0, a.cw - 1);
    const int wx0 = LEFT ? ((fx & 1) ? 2 : 4) : 3, wx1 = 4 - wx0;
    const long long i00 = (long long)r0 * a.cw + q0, i01 = (long long)r0 * a.cw + q1, i10 = (long long)r1 * a.cw + q0,
                    i11 = (long long)r1 * a.cw + q1;
    const int U = chroma_mix(sample<DEPTH, false>(a.yuv, a.uoff + i00), sample<DEPTH, false>(a.yuv, a.uoff + i01),
                             sample<DEPTH, false>(a.yuv, a.uoff + i10), sample<DEPTH, false>(a.yuv, a.uoff + i11), wx0, wx1);
    const int V = chroma_mix(sample<DEPTH, false>(a.yuv, a.voff + i00), sample<DEPTH, false>(a.yuv, a.voff + i01),
                             sample<DEPTH, false>(a.yuv, a.voff + i10), sample<DEPTH, false>(a.yuv, a.voff + i11), wx0, wx1);
    to_rgb(a, sample<DEPTH, false>(a.yuv, (long long)fy * a.W + fx), U, V, q);
}

// four frame pixels of row fy, columns gx .. gx + 3 (gx even, the row's Y group readable as dwords) from the chroma segments of rows
// r0 / r1, seg[k] = column clamp((gx >> 1) - 1 + k) (the aligned paths)
template <int DEPTH, bool LEFT>
__device__ __forceinline__ void decode4(const YuvSrc& a, int fy, int gx, const int u0[4], const int u1[4], const int v0[4], const int v1[4],
                                        int q[4][3]) {
    int Y[4];
    if (DEPTH == 8) {
        const unsigned d = *reinterpret_cast<const unsigned*>(a.yuv + (long long)fy * a.W + gx);
#pragma unroll
        for (int i = 0; i < 4; ++i) Y[i] = (int)((d >> (8 * i)) & 0xffu);
    } else {
        const U32x2 d = *reinterpret_cast<const U32x2*>(a.yuv + 2 * ((long long)fy * a.W + gx));
        Y[0] = (int)(d.a & 0xffffu);
        Y[1] = (int)(d.a >> 16);
        Y[2] = (int)(d.b & 0xffffu);
        Y[3] = (int)(d.b >> 16);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k0 = 1 + (i >> 1);
        const int k1 = LEFT ? k0 + 1 : k0 + ((i & 1) ? 1 : -1);        // (indices and weights are compile-time constants)
        const int wx0 = LEFT ? ((i & 1) ? 2 : 4) : 3, wx1 = 4 - wx0;
        const int U = chroma_mix(u0[k0], u0[k1], u1[k0], u1[k1], wx0, wx1);
        const int V = chroma_mix(v0[k0], v0[k1], v1[k0], v1[k1], wx0, wx1);
        to_rgb(a, Y[i], U, V, q[i]);
    }
}

int check_format(const char* what, int H, int W, int matrix, int full_range, int siting) {
    ATMVFI_REQUIRE(H >= 1 && W >= 1, ATMVFI_EINVAL, "%s: H and W must be at least 1 (got %d x %d)", what, H, W);
    ATMVFI_REQUIRE(matrix == 0 || matrix == 1, ATMVFI_EINVAL, "%s: unknown matrix %d (0: bt601, 1: bt709)", what, matrix);
    ATMVFI_REQUIRE(full_range == 0 || full_range == 1, ATMVFI_EINVAL, "%s: full_range must be 0 or 1 (got %d)", what, full_range);
    ATMVFI_REQUIRE(siting == 0 || siting == 1, ATMVFI_EINVAL, "%s: unknown siting %d (0: centre, 1: left)", what, siting);
    return ATMVFI_OK;
}

}  // namespace
