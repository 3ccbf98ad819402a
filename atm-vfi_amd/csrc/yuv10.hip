// 10-bit planar YUV 4:2:0 (I420, little-endian uint16 samples 0..1023, limited range) <-> fp32 planar RGB with the depth kept:
// atmvfi_yuv420p10_to_f32 / atmvfi_f32_to_yuv420p10 (include/atmvfi.h; atm-vfi_amd/yuv.py holds the numpy twins decode_numpy_f32 /
// encode_numpy).  yuv.hip's structure with 10-bit pixels on both sides: where yuv.hip decodes 10-bit samples to clip8 RGB (q / 255) and
// encodes 8-bit frames only, these calls hand the network q / 1023 and write its prediction back as 10-bit samples.  Nothing of the
// reference: its scripts take PNGs.  The definition is the project's own, in int32 throughout (>> floors), so the device, the numpy twins
// and the per-pixel model (tests/cpu_yuv10.py) agree bit for bit.
//   frame     Y [H,W], U [ch,cw], V [ch,cw] back to back, ch = (H + 1) / 2, cw = (W + 1) / 2
//   decode    chroma upsampling is yuv.hip's, on the 10-bit samples: rows r0 = y >> 1, r1 = clamp(r0 + (y & 1 ? 1 : -1)), weights (3, 1);
//             columns centre-sited q0 = x >> 1, q1 = clamp(q0 + (x & 1 ? 1 : -1)), weights (3, 1); left-sited q1 = min(q0 + 1, cw - 1),
//             weights (4, 0) for even and (2, 2) for odd x; c' = (.. + 8) >> 4.  y = Y - 64, u = U' - 512, v = V' - 512;
//             R = clip10((kY y + kRV v + 2^13) >> 14), G = clip10((kY y + kGU u + kGV v + 2^13) >> 14), B = clip10((kY y + kBU u + 2^13) >> 14);
//             the output is q / 1023 with the bits of the fp32 division.  The call decodes the window (y0, x0, h, w) of the frame (even
//             origin) to (pad_top, pad_left) of the canvas, replicate padding by clamping the output coordinate INTO THE WINDOW; chroma
//             neighbours clamp at the FRAME's edges: the window is a window of the whole frame's decode.
//   encode    source pixel p = clip10(rint(fl32(x * 1023))), half to even; Y = clip10(((eY . p + 2^13) >> 14) + 64); chroma sample (j, i)
//             from the un-rounded sums s with yuv.hip's taps (centre: 2 x 2, sh = 2; left: 1-2-1 x 2, sh = 3):
//             U = clip10(((eU . s + 2^(13 + sh)) >> (14 + sh)) + 512), V alike
//
// Bandwidth-bound: decode moves 3 B/px in and 12 out, encode 12 in and 3 out.  A lane owns a 4 x 2 luma block, as in yuv.hip.
//   vector path (frame pointer 4-byte aligned, W % 4 == 0; the fp32 canvas 16-byte aligned with Wp % 4 == 0 and pad_left % 4 == 0; for
//           the decode also x0 % 4 == 0 and w % 4 == 0): four Y samples are one 8-byte access, a chroma pair one dword, a plane group
//           one 16-byte store or load;
//   general path: any geometry and alignment: byte accesses to the frame, scalar fp32 accesses, the same integer arithmetic, the same bits.
// Vector stores only, no atomics, nothing pre-zeroed: every output byte and word is written by exactly one lane.
#include "common.h"

namespace {

struct alignas(4) U32x2 {
    unsigned a, b;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clip10(int v) { return v < 0 ? 0 : (v > 1023 ? 1023 : v); }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// rint(c * 2^14) of the float64 matrices of (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722), luma scaled by 876 / 1023 and chroma by
// 896 / 1023 (yuv.py derives them again: COEFFS10; tests/test_yuv10_cpu.py holds both to the table of the README and the header)
struct Coeffs10 {
    int dec[5];         // kY, kRV, kGU, kGV, kBU
    int enc[3][3];      // rows Y, U, V over (R, G, B)
};
const Coeffs10 kCoeffs10[2] = {     // [matrix]
    {{19133, 26226, -6438, -13359, 33148}, {{4195, 8235, 1599}, {-2421, -4754, 7175}, {7175, -6008, -1167}}},
    {{19133, 29459, -3504, -8757, 34711}, {{2983, 10034, 1013}, {-1644, -5531, 7175}, {7175, -6517, -658}}},
};

// ------------------------------------------------------------------------------------------------------------------------ decode
struct Dec10Args {
    const unsigned char* yuv;
    int H, W, ch, cw;           // the whole frame
    long long uoff, voff;       // first U / V sample, in samples
    int kY, kRV, kGU, kGV, kBU;
    int y0, x0, h, w;           // the window
    float* dst;
    int Hp, Wp, pad_top, pad_left;
    int groups;                 // ceil(Wp / 4)
    int pairs;                  // ceil(Hp / 2)
};

template <bool AL>
__device__ __forceinline__ int sample10(const unsigned char* p, long long i) {
    if (AL) return reinterpret_cast<const unsigned short*>(p)[i];
    return (int)p[2 * i] | ((int)p[2 * i + 1] << 8);
}

// seg[k] = plane[r][clamp(q - 1 + k, 0, cw - 1)], k = 0..3: every chroma column that luma columns 2q .. 2q + 3 touch (vector path:
// q even and cw even, so (q, q + 1) is a naturally aligned dword inside the row)
__device__ __forceinline__ void load_seg10(const Dec10Args& a, long long plane, int r, int q, int seg[4]) {
    const long long row = plane + (long long)r * a.cw;
    seg[0] = sample10<true>(a.yuv, row + max(q - 1, 0));
    const unsigned v = *reinterpret_cast<const unsigned*>(a.yuv + 2 * (row + q));
    seg[1] = (int)(v & 0xffffu);
    seg[2] = (int)(v >> 16);
    seg[3] = sample10<true>(a.yuv, row + min(q + 2, a.cw - 1));
}

// q / 1023 for an integer q in 0..1023 with the bits of the fp32 division: q * r with r = fl(1 / 1023), then one correction step in
// fused multiply-adds -- e = fl(q - 1023 y), y + e r (yuv.hip's q255 with the other divisor).  Equal to the division for all 1024
// values: tests/test_yuv10_cpu.py checks every one in exact rational arithmetic.
__device__ __forceinline__ float q1023(int q) {
    const float f = (float)q, r = 0x1.00401p-10f;
    const float y = f * r;
    return __fmaf_rn(__fmaf_rn(-1023.0f, y, f), r, y);
}

__device__ __forceinline__ int chroma_mix10(int c00, int c01, int c10, int c11, int wx0, int wx1) {
    return (3 * (wx0 * c00 + wx1 * c01) + (wx0 * c10 + wx1 * c11) + 8) >> 4;
}

// (__mul24: the full-rate 24-bit multiply; coefficients are below 2^17 and samples below 2^14, so the low 32 bits are the product's)
__device__ __forceinline__ void to_rgb10(const Dec10Args& a, int Y, int U, int V, int q[3]) {
    const int y = __mul24(a.kY, Y - 64), u = U - 512, v = V - 512, half = 1 << 13;
    q[0] = clip10((y + __mul24(a.kRV, v) + half) >> 14);
    q[1] = clip10((y + __mul24(a.kGU, u) + __mul24(a.kGV, v) + half) >> 14);
    q[2] = clip10((y + __mul24(a.kBU, u) + half) >> 14);
}

// one frame pixel, every sample loaded on its own, byte by byte (the general path)
template <bool LEFT>
__device__ __forceinline__ void decode_pixel10(const Dec10Args& a, int fy, int fx, int q[3]) {
    const int r0 = fy >> 1, r1 = clampi(r0 + ((fy & 1) ? 1 : -1), 0, a.ch - 1);
    const int q0 = fx >> 1;
    const int q1 = LEFT ? min(q0 + 1, a.cw - 1) : clampi(q0 + ((fx & 1) ? 1 : -1), 0, a.cw - 1);
    const int wx0 = LEFT ? ((fx & 1) ? 2 : 4) : 3, wx1 = 4 - wx0;
    const long long i00 = (long long)r0 * a.cw + q0, i01 = (long long)r0 * a.cw + q1, i10 = (long long)r1 * a.cw + q0,
                    i11 = (long long)r1 * a.cw + q1;
    const int U = chroma_mix10(sample10<false>(a.yuv, a.uoff + i00), sample10<false>(a.yuv, a.uoff + i01),
                               sample10<false>(a.yuv, a.uoff + i10), sample10<false>(a.yuv, a.uoff + i11), wx0, wx1);
    const int V = chroma_mix10(sample10<false>(a.yuv, a.voff + i00), sample10<false>(a.yuv, a.voff + i01),
                               sample10<false>(a.yuv, a.voff + i10), sample10<false>(a.yuv, a.voff + i11), wx0, wx1);
    to_rgb10(a, sample10<false>(a.yuv, (long long)fy * a.W + fx), U, V, q);
}

// four pixels of output row y (frame row fy, frame columns gx .. gx + 3, gx % 4 == 0) from the chroma segments of rows r0 / r1 (vector path)
template <bool LEFT>
__device__ __forceinline__ void decode_group10(const Dec10Args& a, int y, int x, int fy, int gx, bool in, int wx, const int u0[4],
                                               const int u1[4], const int v0[4], const int v1[4]) {
    const U32x2 d = *reinterpret_cast<const U32x2*>(a.yuv + 2 * ((long long)fy * a.W + gx));
    const int Y[4] = {(int)(d.a & 0xffffu), (int)(d.a >> 16), (int)(d.b & 0xffffu), (int)(d.b >> 16)};
    int q[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k0 = 1 + (i >> 1);
        const int k1 = LEFT ? k0 + 1 : k0 + ((i & 1) ? 1 : -1);        // (indices and weights are compile-time constants)
        const int wx0 = LEFT ? ((i & 1) ? 2 : 4) : 3, wx1 = 4 - wx0;
        const int U = chroma_mix10(u0[k0], u0[k1], u1[k0], u1[k1], wx0, wx1);
        const int V = chroma_mix10(v0[k0], v0[k1], v1[k0], v1[k1], wx0, wx1);
        to_rgb10(a, Y[i], U, V, q[i]);
    }
    if (!in) {          // left padding repeats the first pixel of the window's first group, right padding the last of its last
#pragma unroll
        for (int c = 0; c < 3; ++c) q[0][c] = q[1][c] = q[2][c] = q[3][c] = wx < 0 ? q[0][c] : q[3][c];
    }
    const long long plane = (long long)a.Hp * a.Wp;
    float* o = a.dst + (long long)y * a.Wp + x;
    *reinterpret_cast<f32x4*>(o) = (f32x4){q1023(q[0][0]), q1023(q[1][0]), q1023(q[2][0]), q1023(q[3][0])};
    *reinterpret_cast<f32x4*>(o + plane) = (f32x4){q1023(q[0][1]), q1023(q[1][1]), q1023(q[2][1]), q1023(q[3][1])};
    *reinterpret_cast<f32x4*>(o + 2 * plane) = (f32x4){q1023(q[0][2]), q1023(q[1][2]), q1023(q[2][2]), q1023(q[3][2])};
}

template <bool ALIGNED, bool LEFT>
__global__ __launch_bounds__(256) void yuv420p10_to_f32_kernel(const Dec10Args a) {
    const long long plane = (long long)a.Hp * a.Wp;
    const int total = a.pairs * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int k = idx / a.groups, x = (idx - k * a.groups) * 4;
        const int wx = x - a.pad_left;                      // window column of the group's first pixel; outside = padding
        if (ALIGNED) {
            const int gx = a.x0 + clampi(wx, 0, a.w - 4), q = gx >> 1;
            const bool in = wx >= 0 && wx < a.w;
            const int yA = 2 * k, yB = yA + 1;
            const int fyA = a.y0 + clampi(yA - a.pad_top, 0, a.h - 1), fyB = a.y0 + clampi(yB - a.pad_top, 0, a.h - 1);
            const int rA0 = fyA >> 1, rA1 = clampi(rA0 + ((fyA & 1) ? 1 : -1), 0, a.ch - 1);
            int uA0[4], uA1[4], vA0[4], vA1[4];
            load_seg10(a, a.uoff, rA0, q, uA0);
            load_seg10(a, a.voff, rA0, q, vA0);
            load_seg10(a, a.uoff, rA1, q, uA1);
            load_seg10(a, a.voff, rA1, q, vA1);
            decode_group10<LEFT>(a, yA, x, fyA, gx, in, wx, uA0, uA1, vA0, vA1);
            if (yB < a.Hp) {
                const int rB0 = fyB >> 1, rB1 = clampi(rB0 + ((fyB & 1) ? 1 : -1), 0, a.ch - 1);
                int uB0[4], uB1[4], vB0[4], vB1[4];
                // a chroma row both luma rows use is already here: inside the frame one of row B's two rows always is
                if (rB0 == rA0 || rB0 == rA1) {
                    const bool f = rB0 == rA0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        uB0[i] = f ? uA0[i] : uA1[i];
                        vB0[i] = f ? vA0[i] : vA1[i];
                    }
                } else {
                    load_seg10(a, a.uoff, rB0, q, uB0);
                    load_seg10(a, a.voff, rB0, q, vB0);
                }
                if (rB1 == rA0 || rB1 == rA1) {
                    const bool f = rB1 == rA0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        uB1[i] = f ? uA0[i] : uA1[i];
                        vB1[i] = f ? vA0[i] : vA1[i];
                    }
                } else {
                    load_seg10(a, a.uoff, rB1, q, uB1);
                    load_seg10(a, a.voff, rB1, q, vB1);
                }
                decode_group10<LEFT>(a, yB, x, fyB, gx, in, wx, uB0, uB1, vB0, vB1);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = 2 * k + r;
                if (y >= a.Hp) break;
                const int fy = a.y0 + clampi(y - a.pad_top, 0, a.h - 1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (x + i >= a.Wp) break;
                    int q[3];
                    decode_pixel10<LEFT>(a, fy, a.x0 + clampi(wx + i, 0, a.w - 1), q);
                    float* o = a.dst + (long long)y * a.Wp + x + i;
                    o[0] = q1023(q[0]);
                    o[plane] = q1023(q[1]);
                    o[2 * plane] = q1023(q[2]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ encode
struct Enc10Args {
    const float* src;
    int Hp, Wp, pad_top, pad_left;
    int H, W, ch, cw;
    int eY[3], eU[3], eV[3];
    unsigned char* yuv;
    long long uoff, voff;       // in samples
    int groups;                 // ceil(W / 4); a group makes chroma columns 2g and 2g + 1
};

__device__ __forceinline__ int f32_to_q10(float v) {
    return clip10(__float2int_rn(v * 1023.0f));        // rint: half to even, as np.rint; the conversion saturates
}

__device__ __forceinline__ void load_px10(const Enc10Args& a, int fy, int fx, int p[3]) {
    const long long plane = (long long)a.Hp * a.Wp;
    const float* s = a.src + (long long)(fy + a.pad_top) * a.Wp + (fx + a.pad_left);
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = f32_to_q10(s[c * plane]);
}

__device__ __forceinline__ void load_px4_aligned10(const Enc10Args& a, int fy, int fx, int p[4][3]) {
    const long long plane = (long long)a.Hp * a.Wp;
    const float* s = a.src + (long long)(fy + a.pad_top) * a.Wp + (fx + a.pad_left);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + c * plane);
        p[0][c] = f32_to_q10(v.x);
        p[1][c] = f32_to_q10(v.y);
        p[2][c] = f32_to_q10(v.z);
        p[3][c] = f32_to_q10(v.w);
    }
}

// (__mul24: coefficients are below 2^14 and pixel sums below 2^14)
__device__ __forceinline__ int dot3_10(const int e[3], const int p[3]) {
    return __mul24(e[0], p[0]) + __mul24(e[1], p[1]) + __mul24(e[2], p[2]);
}

__device__ __forceinline__ void store_sample10(unsigned char* yuv, long long i, int v) {
    yuv[2 * i] = (unsigned char)(v & 0xff);
    yuv[2 * i + 1] = (unsigned char)(v >> 8);
}

template <bool ALIGNED, bool LEFT>
__global__ __launch_bounds__(256) void f32_to_yuv420p10_kernel(const Enc10Args a) {
    const int total = a.ch * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int j = idx / a.groups, g = idx - j * a.groups, x = 4 * g;
        int px[2][5][3];        // [row][0: the column left of the group (left siting only), 1..4: the group][R, G, B]
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int fy = min(2 * j + r, a.H - 1);
            if (ALIGNED) {
                load_px4_aligned10(a, fy, x, &px[r][1]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) load_px10(a, fy, min(x + i, a.W - 1), px[r][1 + i]);
            }
            if (LEFT) load_px10(a, fy, max(x - 1, 0), px[r][0]);
            else px[r][0][0] = px[r][0][1] = px[r][0][2] = 0;
        }
        // luma
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * j + r;
            if (y >= a.H) break;
            int Y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) Y[i] = clip10(((dot3_10(a.eY, px[r][1 + i]) + (1 << 13)) >> 14) + 64);
            const long long o = (long long)y * a.W + x;
            if (ALIGNED) {
                *reinterpret_cast<U32x2*>(a.yuv + 2 * o) = U32x2{(unsigned)Y[0] | ((unsigned)Y[1] << 16), (unsigned)Y[2] | ((unsigned)Y[3] << 16)};
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x + i < a.W) store_sample10(a.yuv, o + i, Y[i]);
            }
        }
        // chroma columns 2g and 2g + 1
        const int sh = LEFT ? 3 : 2;
        int U[2], V[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (LEFT)
                    s[c] = px[0][2 * i][c] + 2 * px[0][1 + 2 * i][c] + px[0][2 + 2 * i][c] + px[1][2 * i][c] + 2 * px[1][1 + 2 * i][c] +
                           px[1][2 + 2 * i][c];
                else
                    s[c] = px[0][1 + 2 * i][c] + px[0][2 + 2 * i][c] + px[1][1 + 2 * i][c] + px[1][2 + 2 * i][c];
            }
            U[i] = clip10(((dot3_10(a.eU, s) + (1 << (13 + sh))) >> (14 + sh)) + 512);
            V[i] = clip10(((dot3_10(a.eV, s) + (1 << (13 + sh))) >> (14 + sh)) + 512);
        }
        const long long c0 = (long long)j * a.cw + 2 * g;
        if (ALIGNED) {          // cw even: both columns exist and the pair is a naturally aligned dword
            *reinterpret_cast<unsigned*>(a.yuv + 2 * (a.uoff + c0)) = (unsigned)U[0] | ((unsigned)U[1] << 16);
            *reinterpret_cast<unsigned*>(a.yuv + 2 * (a.voff + c0)) = (unsigned)V[0] | ((unsigned)V[1] << 16);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (2 * g + i < a.cw) {
                    store_sample10(a.yuv, a.uoff + c0 + i, U[i]);
                    store_sample10(a.yuv, a.voff + c0 + i, V[i]);
                }
            }
        }
    }
}

int check_format10(const char* what, int H, int W, int matrix, int siting) {
    ATMVFI_REQUIRE(H >= 1 && W >= 1, ATMVFI_EINVAL, "%s: H and W must be at least 1 (got %d x %d)", what, H, W);
    ATMVFI_REQUIRE(matrix == 0 || matrix == 1, ATMVFI_EINVAL, "%s: unknown matrix %d (0: bt601, 1: bt709)", what, matrix);
    ATMVFI_REQUIRE(siting == 0 || siting == 1, ATMVFI_EINVAL, "%s: unknown siting %d (0: centre, 1: left)", what, siting);
    return ATMVFI_OK;
}

}  // namespace

extern "C" int atmvfi_yuv420p10_to_f32(const void* yuv, int H, int W, int matrix, int siting, int y0, int x0, int h, int w, float* dst,
                                       int Hp, int Wp, int pad_top, int pad_left, void* stream) {
    ATMVFI_REQUIRE(yuv, ATMVFI_EINVAL, "yuv420p10_to_f32: null source");
    ATMVFI_REQUIRE(dst, ATMVFI_EINVAL, "yuv420p10_to_f32: null destination");
    if (const int rc = check_format10("yuv420p10_to_f32", H, W, matrix, siting)) return rc;
    ATMVFI_REQUIRE(h >= 1 && w >= 1, ATMVFI_EINVAL, "yuv420p10_to_f32: the window's h and w must be at least 1 (got %d x %d)", h, w);
    ATMVFI_REQUIRE(y0 >= 0 && x0 >= 0 && (long long)y0 + h <= H && (long long)x0 + w <= W, ATMVFI_EINVAL,
                   "yuv420p10_to_f32: window %d x %d at (%d, %d) outside the %d x %d frame", h, w, y0, x0, H, W);
    ATMVFI_REQUIRE(y0 % 2 == 0 && x0 % 2 == 0, ATMVFI_EINVAL, "yuv420p10_to_f32: the window origin (%d, %d) must be even", y0, x0);
    ATMVFI_REQUIRE(aligned4(dst), ATMVFI_EINVAL, "yuv420p10_to_f32: dst must be 4-byte aligned");
    ATMVFI_REQUIRE(pad_top >= 0 && pad_left >= 0 && (long long)h + pad_top <= Hp && (long long)w + pad_left <= Wp, ATMVFI_EINVAL,
                   "yuv420p10_to_f32: canvas %d x %d is smaller than the window %d x %d plus padding (%d, %d)", Hp, Wp, h, w, pad_top,
                   pad_left);
    const int groups = (int)(((long long)Wp + 3) / 4), pairs = (int)(((long long)Hp + 1) / 2);
    ATMVFI_REQUIRE((long long)pairs * groups < (1ll << 30), ATMVFI_EINVAL, "yuv420p10_to_f32: output of %d x %d is too large", Hp, Wp);
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;
    const Coeffs10& c = kCoeffs10[matrix];
    const Dec10Args a = {(const unsigned char*)yuv, H, W, ch, cw, (long long)H * W, (long long)H * W + (long long)ch * cw,
                         c.dec[0], c.dec[1], c.dec[2], c.dec[3], c.dec[4], y0, x0, h, w, dst, Hp, Wp, pad_top, pad_left, groups, pairs};
    // vector path: Y groups are 8-byte loads, chroma pairs naturally aligned dwords (cw even), plane stores 16 bytes; a group of four
    // lies wholly inside the window or wholly in the padding
    const bool al = aligned4(yuv) && W % 4 == 0 && x0 % 4 == 0 && w % 4 == 0 && pad_left % 4 == 0 && Wp % 4 == 0 && atmvfi::aligned16(dst);
    const long long blocks = ((long long)pairs * groups + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    // the siting is a template parameter: the tap indices and weights of the chroma filter are constants of the instance
    if (al) {
        if (siting) hipLaunchKernelGGL((yuv420p10_to_f32_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((yuv420p10_to_f32_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (siting) hipLaunchKernelGGL((yuv420p10_to_f32_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((yuv420p10_to_f32_kernel<false, false>), grid, block, 0, st, a);
    }
    return atmvfi::check_launch("yuv420p10_to_f32");
}

extern "C" int atmvfi_f32_to_yuv420p10(const float* src, int Hp, int Wp, int pad_top, int pad_left, int H, int W, int matrix, int siting,
                                       void* yuv, void* stream) {
    ATMVFI_REQUIRE(src, ATMVFI_EINVAL, "f32_to_yuv420p10: null source");
    ATMVFI_REQUIRE(yuv, ATMVFI_EINVAL, "f32_to_yuv420p10: null destination");
    if (const int rc = check_format10("f32_to_yuv420p10", H, W, matrix, siting)) return rc;
    ATMVFI_REQUIRE(aligned4(src), ATMVFI_EINVAL, "f32_to_yuv420p10: src must be 4-byte aligned");
    ATMVFI_REQUIRE(pad_top >= 0 && pad_left >= 0 && (long long)H + pad_top <= Hp && (long long)W + pad_left <= Wp, ATMVFI_EINVAL,
                   "f32_to_yuv420p10: canvas %d x %d is smaller than the frame %d x %d plus padding (%d, %d)", Hp, Wp, H, W, pad_top,
                   pad_left);
    const int ch = (H + 1) / 2, cw = (W + 1) / 2, groups = (int)(((long long)W + 3) / 4);
    ATMVFI_REQUIRE((long long)ch * groups < (1ll << 30), ATMVFI_EINVAL, "f32_to_yuv420p10: a frame of %d x %d is too large", H, W);
    const Coeffs10& c = kCoeffs10[matrix];
    Enc10Args a = {};
    a.src = src;
    a.Hp = Hp; a.Wp = Wp; a.pad_top = pad_top; a.pad_left = pad_left;
    a.H = H; a.W = W; a.ch = ch; a.cw = cw;
    for (int k = 0; k < 3; ++k) {
        a.eY[k] = c.enc[0][k];
        a.eU[k] = c.enc[1][k];
        a.eV[k] = c.enc[2][k];
    }
    a.yuv = (unsigned char*)yuv;
    a.uoff = (long long)H * W;
    a.voff = a.uoff + (long long)ch * cw;
    a.groups = groups;
    // vector path: Y groups are 8-byte stores, chroma pairs dword stores (cw even), the source group three 16-byte loads
    const bool al = aligned4(yuv) && W % 4 == 0 && atmvfi::aligned16(src) && Wp % 4 == 0 && pad_left % 4 == 0;
    const long long blocks = ((long long)ch * groups + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (al) {
        if (siting) hipLaunchKernelGGL((f32_to_yuv420p10_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((f32_to_yuv420p10_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (siting) hipLaunchKernelGGL((f32_to_yuv420p10_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((f32_to_yuv420p10_kernel<false, false>), grid, block, 0, st, a);
    }
    return atmvfi::check_launch("f32_to_yuv420p10");
}
