// Planar YUV 4:2:0 (I420) <-> RGB at the host boundary of the video loops (include/atmvfi.h, atmvfi_yuv420_to_rgb / atmvfi_rgb_to_yuv420;
// atm-vfi_amd/yuv.py holds the numpy twins).  Nothing of the reference: its scripts take PNGs.  The definition is the project's own, in
// int32 throughout, so the device, the vectorised numpy twins and the per-pixel model (tests/cpu_yuv.py) agree bit for bit.
//   frame     Y [H,W], U [ch,cw], V [ch,cw] back to back, ch = (H + 1) / 2, cw = (W + 1) / 2; uint8, or little-endian uint16 (0..1023)
//             for depth 10 (decode only)
//   decode    chroma of luma pixel (y, x): rows r0 = y >> 1 and r1 = clamp(r0 + (y & 1 ? 1 : -1)) with weights (3, 1); columns
//             centre-sited q0 = x >> 1, q1 = clamp(q0 + (x & 1 ? 1 : -1)), weights (3, 1); left-sited q0, q1 = min(q0 + 1, cw - 1),
//             weights (4, 0) for even and (2, 2) for odd x; c' = (wy0 (wx0 c00 + wx1 c01) + wy1 (wx0 c10 + wx1 c11) + 8) >> 4;
//             R = clip8((kY y + kRV v + 2^(T-1)) >> T), G = clip8((kY y + kGU u + kGV v + ..) >> T), B = clip8((kY y + kBU u + ..) >> T)
//             with y = Y - yo, u = U' - mid, v = V' - mid; T = 14 (8 bit) or 16 (10 bit)
//   encode    source pixel: the uint8 RGB value, from fp32 clamp(rint(x * 255)) (frame_f32_to_u8's pixel);
//             Y = clip8(((eY . p + 2^13) >> 14) + yo); chroma sample (j, i) from the un-rounded sums s over rows 2j, min(2j + 1, H - 1) and
//             columns 2i, min(2i + 1, W - 1) (centre, sh = 2) or max(2i - 1, 0), 2i, min(2i + 1, W - 1) weighted 1, 2, 1 (left, sh = 3):
//             U = clip8(((eU . s + 2^(13 + sh)) >> (14 + sh)) + 128), V alike
//
// Bandwidth-bound: decode to fp32 moves 1.5 B/px in and 12 out, encode from fp32 12 in and 1.5 out.  A lane owns a 4 x 2 luma block:
//   decode: 4 x 2 pixels of the PADDED output (padding comes from clamping the output coordinate, as in frames.hip).  The two rows need
//           at most three chroma rows, four samples wide (columns q - 1 .. q + 2 of the group, clamped): a row that both luma rows use
//           is loaded once.  Chroma is read straight from global memory: neighbouring lanes and rows re-read the same few bytes, which
//           the vector L1 serves; the HBM traffic is the frame, once.
//   encode: 4 x 2 pixels of the frame -> two Y dwords and two chroma samples per plane; left siting reads one more pixel column.
//   aligned path (frame pointer 4-byte aligned, W % 4 == 0 and, for the fp32 canvas, 16-byte aligned with Wp % 4 == 0 and
//           pad_left % 4 == 0): dword Y loads / stores, 16-byte plane accesses, one 12-byte RGB group per four pixels, 2-byte chroma pairs;
//   general path: any geometry and alignment: byte accesses, the same integer arithmetic, the same bits.
// Vector stores only, no atomics, nothing pre-zeroed: every output byte is written by exactly one lane.
// The depth-keeping 10-bit calls (10-bit samples <-> fp32 in units of 1 / 1023; atmvfi_yuv420p10_to_f32 / atmvfi_f32_to_yuv420p10) live
// in yuv10.hip; the 10-bit decode here stays what it was: clip8 RGB, q / 255.  The decode's device helpers (loads, chroma filter, matrix,
// q / 255) live in yuv_common.h, which yuv_window.hip (atmvfi_yuv420_window) shares.
#include "yuv_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------ decode
struct DecArgs : YuvSrc {      // (yuv_common.h: the frame, its planes and the matrix)
    float* dst;
    int Hp, Wp, pad_top, pad_left;
    unsigned char* dst_u8;
    int bgr;
    int groups;                 // ceil(Wp / 4)
    int pairs;                  // ceil(Hp / 2)
};

// four pixels of output row y (frame row fy, frame columns gx .. gx + 3, gx % 4 == 0) from the chroma segments of rows r0 / r1 (aligned path)
template <int DEPTH, bool LEFT>
__device__ __forceinline__ void decode_group(const DecArgs& a, int y, int x, int fy, int gx, bool in, int wx, const int u0[4],
                                             const int u1[4], const int v0[4], const int v1[4]) {
    int q[4][3];
    decode4<DEPTH, LEFT>(a, fy, gx, u0, u1, v0, v1, q);
    if (!in) {          // left padding repeats the first pixel of the first group, right padding the last of the last
#pragma unroll
        for (int c = 0; c < 3; ++c) q[0][c] = q[1][c] = q[2][c] = q[3][c] = wx < 0 ? q[0][c] : q[3][c];
    }
    if (a.dst) {
        const long long plane = (long long)a.Hp * a.Wp;
        float* o = a.dst + (long long)y * a.Wp + x;
        *reinterpret_cast<f32x4*>(o) = (f32x4){q255(q[0][0]), q255(q[1][0]), q255(q[2][0]), q255(q[3][0])};
        *reinterpret_cast<f32x4*>(o + plane) = (f32x4){q255(q[0][1]), q255(q[1][1]), q255(q[2][1]), q255(q[3][1])};
        *reinterpret_cast<f32x4*>(o + 2 * plane) = (f32x4){q255(q[0][2]), q255(q[1][2]), q255(q[2][2]), q255(q[3][2])};
    }
    const int wy = y - a.pad_top;
    if (a.dst_u8 && in && wy >= 0 && wy < a.H) {
        unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int v = a.bgr ? q[i][2 - c] : q[i][c];
                d[(3 * i + c) >> 2] |= (unsigned)v << (((3 * i + c) & 3) * 8);
            }
        }
        *reinterpret_cast<U32x3*>(a.dst_u8 + ((long long)wy * a.W + wx) * 3) = U32x3{d[0], d[1], d[2]};
    }
}

template <int DEPTH, bool ALIGNED, bool LEFT>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(const DecArgs a) {
    const long long plane = (long long)a.Hp * a.Wp;
    const int total = a.pairs * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int k = idx / a.groups, x = (idx - k * a.groups) * 4;
        const int wx = x - a.pad_left;                      // frame column of the group's first pixel; outside = padding
        if (ALIGNED) {
            const int gx = clampi(wx, 0, a.W - 4), q = gx >> 1;
            const bool in = wx >= 0 && wx < a.W;
            const int yA = 2 * k, yB = yA + 1;
            const int fyA = clampi(yA - a.pad_top, 0, a.H - 1), fyB = clampi(yB - a.pad_top, 0, a.H - 1);
            const int rA0 = fyA >> 1, rA1 = clampi(rA0 + ((fyA & 1) ? 1 : -1), 0, a.ch - 1);
            int uA0[4], uA1[4], vA0[4], vA1[4];
            load_seg<DEPTH, true>(a, a.uoff, rA0, q, uA0);
            load_seg<DEPTH, true>(a, a.voff, rA0, q, vA0);
            load_seg<DEPTH, true>(a, a.uoff, rA1, q, uA1);
            load_seg<DEPTH, true>(a, a.voff, rA1, q, vA1);
            decode_group<DEPTH, LEFT>(a, yA, x, fyA, gx, in, wx, uA0, uA1, vA0, vA1);
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
                    load_seg<DEPTH, true>(a, a.uoff, rB0, q, uB0);
                    load_seg<DEPTH, true>(a, a.voff, rB0, q, vB0);
                }
                if (rB1 == rA0 || rB1 == rA1) {
                    const bool f = rB1 == rA0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        uB1[i] = f ? uA0[i] : uA1[i];
                        vB1[i] = f ? vA0[i] : vA1[i];
                    }
                } else {
                    load_seg<DEPTH, true>(a, a.uoff, rB1, q, uB1);
                    load_seg<DEPTH, true>(a, a.voff, rB1, q, vB1);
                }
                decode_group<DEPTH, LEFT>(a, yB, x, fyB, gx, in, wx, uB0, uB1, vB0, vB1);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = 2 * k + r, wy = y - a.pad_top;
                if (y >= a.Hp) break;
                const int fy = clampi(wy, 0, a.H - 1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (x + i >= a.Wp) break;
                    int q[3];
                    decode_pixel<DEPTH, LEFT>(a, fy, clampi(wx + i, 0, a.W - 1), q);
                    if (a.dst) {
                        float* o = a.dst + (long long)y * a.Wp + x + i;
                        o[0] = q255(q[0]);
                        o[plane] = q255(q[1]);
                        o[2 * plane] = q255(q[2]);
                    }
                    if (a.dst_u8 && wy >= 0 && wy < a.H && wx + i >= 0 && wx + i < a.W) {
                        unsigned char* o = a.dst_u8 + ((long long)wy * a.W + wx + i) * 3;
                        o[0] = (unsigned char)(a.bgr ? q[2] : q[0]);
                        o[1] = (unsigned char)q[1];
                        o[2] = (unsigned char)(a.bgr ? q[0] : q[2]);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ encode
struct EncArgs {
    const unsigned char* src_u8;
    const float* src;
    int Hp, Wp, pad_top, pad_left;
    int H, W, ch, cw;
    int bgr, left;
    int eY[3], eU[3], eV[3], yo;
    unsigned char* yuv;
    long long uoff, voff;
    int groups;                 // ceil(W / 4); a group makes chroma columns 2g and 2g + 1
};

__device__ __forceinline__ int f32_to_q(float v) {
    const int q = __float2int_rn(v * 255.0f);       // rint: half to even, as np.round (frame_f32_to_u8)
    return clip8(q);
}

template <bool F32>
__device__ __forceinline__ void load_px(const EncArgs& a, int fy, int fx, int p[3]) {
    if (F32) {
        const long long plane = (long long)a.Hp * a.Wp;
        const float* s = a.src + (long long)(fy + a.pad_top) * a.Wp + (fx + a.pad_left);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = f32_to_q(s[c * plane]);
    } else {
        const unsigned char* s = a.src_u8 + ((long long)fy * a.W + fx) * 3;
        p[0] = a.bgr ? s[2] : s[0];
        p[1] = s[1];
        p[2] = a.bgr ? s[0] : s[2];
    }
}

template <bool F32>
__device__ __forceinline__ void load_px4_aligned(const EncArgs& a, int fy, int fx, int p[4][3]) {
    if (F32) {
        const long long plane = (long long)a.Hp * a.Wp;
        const float* s = a.src + (long long)(fy + a.pad_top) * a.Wp + (fx + a.pad_left);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(s + c * plane);
            p[0][c] = f32_to_q(v.x);
            p[1][c] = f32_to_q(v.y);
            p[2][c] = f32_to_q(v.z);
            p[3][c] = f32_to_q(v.w);
        }
    } else {
        const U32x3 r = *reinterpret_cast<const U32x3*>(a.src_u8 + ((long long)fy * a.W + fx) * 3);
        const unsigned d[3] = {r.a, r.b, r.c};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int kr = 3 * i + c, kb = 3 * i + 2 - c;       // (a select between two compile-time bytes)
                const int vr = (int)((d[kr >> 2] >> ((kr & 3) * 8)) & 0xffu), vb = (int)((d[kb >> 2] >> ((kb & 3) * 8)) & 0xffu);
                p[i][c] = a.bgr ? vb : vr;
            }
        }
    }
}

// (__mul24: coefficients are below 2^14 and pixel sums below 2^11)
__device__ __forceinline__ int dot3(const int e[3], const int p[3]) { return __mul24(e[0], p[0]) + __mul24(e[1], p[1]) + __mul24(e[2], p[2]); }

template <bool F32, bool ALIGNED>
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const EncArgs a) {
    const int total = a.ch * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int j = idx / a.groups, g = idx - j * a.groups, x = 4 * g;
        int px[2][5][3];        // [row][0: the column left of the group (left siting only), 1..4: the group][R, G, B]
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int fy = min(2 * j + r, a.H - 1);
            if (ALIGNED) {
                load_px4_aligned<F32>(a, fy, x, &px[r][1]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) load_px<F32>(a, fy, min(x + i, a.W - 1), px[r][1 + i]);
            }
            if (a.left) load_px<F32>(a, fy, max(x - 1, 0), px[r][0]);
            else px[r][0][0] = px[r][0][1] = px[r][0][2] = 0;
        }
        // luma
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * j + r;
            if (y >= a.H) break;
            int Y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) Y[i] = clip8(((dot3(a.eY, px[r][1 + i]) + (1 << 13)) >> 14) + a.yo);
            unsigned char* o = a.yuv + (long long)y * a.W + x;
            if (ALIGNED) {
                *reinterpret_cast<unsigned*>(o) = (unsigned)Y[0] | ((unsigned)Y[1] << 8) | ((unsigned)Y[2] << 16) | ((unsigned)Y[3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x + i < a.W) o[i] = (unsigned char)Y[i];
            }
        }
        // chroma columns 2g and 2g + 1
        const int sh = a.left ? 3 : 2;
        int U[2], V[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int centre = px[0][1 + 2 * i][c] + px[0][2 + 2 * i][c] + px[1][1 + 2 * i][c] + px[1][2 + 2 * i][c];
                const int left = px[0][2 * i][c] + 2 * px[0][1 + 2 * i][c] + px[0][2 + 2 * i][c] + px[1][2 * i][c] + 2 * px[1][1 + 2 * i][c] +
                                 px[1][2 + 2 * i][c];
                s[c] = a.left ? left : centre;
            }
            U[i] = clip8(((dot3(a.eU, s) + (1 << (13 + sh))) >> (14 + sh)) + 128);
            V[i] = clip8(((dot3(a.eV, s) + (1 << (13 + sh))) >> (14 + sh)) + 128);
        }
        const long long c0 = (long long)j * a.cw + 2 * g;
        if (ALIGNED) {          // cw even: both columns exist and the pair is 2-byte aligned
            reinterpret_cast<U16x1*>(a.yuv + a.uoff + c0)->v = (unsigned short)(U[0] | (U[1] << 8));
            reinterpret_cast<U16x1*>(a.yuv + a.voff + c0)->v = (unsigned short)(V[0] | (V[1] << 8));
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (2 * g + i < a.cw) {
                    a.yuv[a.uoff + c0 + i] = (unsigned char)U[i];
                    a.yuv[a.voff + c0 + i] = (unsigned char)V[i];
                }
            }
        }
    }
}


}  // namespace

extern "C" int atmvfi_yuv420_to_rgb(const void* yuv, int H, int W, int depth, int matrix, int full_range, int siting, void* dst_u8, int bgr,
                                    float* dst, int Hp, int Wp, int pad_top, int pad_left, void* stream) {
    ATMVFI_REQUIRE(yuv, ATMVFI_EINVAL, "yuv420_to_rgb: null source");
    ATMVFI_REQUIRE(dst || dst_u8, ATMVFI_EINVAL, "yuv420_to_rgb: both outputs are null (give dst, dst_u8 or both)");
    if (const int rc = check_format("yuv420_to_rgb", H, W, matrix, full_range, siting)) return rc;
    ATMVFI_REQUIRE(depth == 8 || depth == 10, ATMVFI_EINVAL, "yuv420_to_rgb: depth must be 8 or 10 (got %d)", depth);
    ATMVFI_REQUIRE(!(depth == 10 && full_range), ATMVFI_EINVAL, "yuv420_to_rgb: 10-bit full range is not supported");
    if (dst) {
        ATMVFI_REQUIRE(aligned4(dst), ATMVFI_EINVAL, "yuv420_to_rgb: dst must be 4-byte aligned");
        ATMVFI_REQUIRE(pad_top >= 0 && pad_left >= 0 && (long long)H + pad_top <= Hp && (long long)W + pad_left <= Wp, ATMVFI_EINVAL,
                       "yuv420_to_rgb: canvas %d x %d is smaller than the frame %d x %d plus padding (%d, %d)", Hp, Wp, H, W, pad_top,
                       pad_left);
    } else {        // no canvas: the output geometry is the frame's
        Hp = H;
        Wp = W;
        pad_top = pad_left = 0;
    }
    const int groups = (int)(((long long)Wp + 3) / 4), pairs = (int)(((long long)Hp + 1) / 2);
    ATMVFI_REQUIRE((long long)pairs * groups < (1ll << 30), ATMVFI_EINVAL, "yuv420_to_rgb: output of %d x %d is too large", Hp, Wp);
    const DecArgs a = {make_src(yuv, H, W, depth, matrix, full_range), dst, Hp, Wp, pad_top, pad_left, (unsigned char*)dst_u8, bgr ? 1 : 0,
                       groups, pairs};
    // aligned path: Y groups are dwords, chroma pairs naturally aligned (cw even), plane stores 16 bytes, RGB groups three dwords;
    // a group of four lies wholly inside the frame or wholly in the padding
    const bool al = aligned4(yuv) && W % 4 == 0 && pad_left % 4 == 0 && Wp % 4 == 0 && (!dst || atmvfi::aligned16(dst)) &&
                    (!dst_u8 || aligned4(dst_u8));
    const long long blocks = ((long long)pairs * groups + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    // the siting is a template parameter: the tap indices and weights of the chroma filter are constants of the instance
#define ATMVFI_YUV_DECODE(DEPTH, AL)                                                                                   \
    do {                                                                                                               \
        if (siting) hipLaunchKernelGGL((yuv420_to_rgb_kernel<DEPTH, AL, true>), grid, block, 0, st, a);                \
        else hipLaunchKernelGGL((yuv420_to_rgb_kernel<DEPTH, AL, false>), grid, block, 0, st, a);                      \
    } while (0)
    if (depth == 8) {
        if (al) ATMVFI_YUV_DECODE(8, true);
        else ATMVFI_YUV_DECODE(8, false);
    } else {
        if (al) ATMVFI_YUV_DECODE(10, true);
        else ATMVFI_YUV_DECODE(10, false);
    }
#undef ATMVFI_YUV_DECODE
    return atmvfi::check_launch("yuv420_to_rgb");
}

extern "C" int atmvfi_rgb_to_yuv420(const void* src_u8, int bgr, const float* src, int Hp, int Wp, int pad_top, int pad_left, int H, int W,
                                    int matrix, int full_range, int siting, void* yuv, void* stream) {
    ATMVFI_REQUIRE(yuv, ATMVFI_EINVAL, "rgb_to_yuv420: null destination");
    ATMVFI_REQUIRE((src_u8 != nullptr) != (src != nullptr), ATMVFI_EINVAL,
                   "rgb_to_yuv420: give exactly one of src_u8 and src (got %s)", src_u8 ? "both" : "neither");
    if (const int rc = check_format("rgb_to_yuv420", H, W, matrix, full_range, siting)) return rc;
    if (src) {
        ATMVFI_REQUIRE(aligned4(src), ATMVFI_EINVAL, "rgb_to_yuv420: src must be 4-byte aligned");
        ATMVFI_REQUIRE(pad_top >= 0 && pad_left >= 0 && (long long)H + pad_top <= Hp && (long long)W + pad_left <= Wp, ATMVFI_EINVAL,
                       "rgb_to_yuv420: canvas %d x %d is smaller than the frame %d x %d plus padding (%d, %d)", Hp, Wp, H, W, pad_top,
                       pad_left);
    }
    const int ch = (H + 1) / 2, cw = (W + 1) / 2, groups = (int)(((long long)W + 3) / 4);
    ATMVFI_REQUIRE((long long)ch * groups < (1ll << 30), ATMVFI_EINVAL, "rgb_to_yuv420: a frame of %d x %d is too large", H, W);
    const Coeffs& c = kCoeffs[matrix][full_range];
    EncArgs a = {};
    a.src_u8 = (const unsigned char*)src_u8;
    a.src = src;
    a.Hp = Hp; a.Wp = Wp; a.pad_top = pad_top; a.pad_left = pad_left;
    a.H = H; a.W = W; a.ch = ch; a.cw = cw;
    a.bgr = bgr ? 1 : 0;
    a.left = siting;
    for (int k = 0; k < 3; ++k) {
        a.eY[k] = c.enc[0][k];
        a.eU[k] = c.enc[1][k];
        a.eV[k] = c.enc[2][k];
    }
    a.yo = full_range ? 0 : 16;
    a.yuv = (unsigned char*)yuv;
    a.uoff = (long long)H * W;
    a.voff = a.uoff + (long long)ch * cw;
    a.groups = groups;
    // aligned path: Y groups are dword stores, chroma pairs 2-byte stores (cw even); the source group is three dwords or three 16-byte loads
    const bool al = aligned4(yuv) && W % 4 == 0 &&
                    (src ? (atmvfi::aligned16(src) && Wp % 4 == 0 && pad_left % 4 == 0) : aligned4(src_u8));
    const long long blocks = ((long long)ch * groups + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (src) {
        if (al) hipLaunchKernelGGL((rgb_to_yuv420_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((rgb_to_yuv420_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (al) hipLaunchKernelGGL((rgb_to_yuv420_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((rgb_to_yuv420_kernel<false, false>), grid, block, 0, st, a);
    }
    return atmvfi::check_launch("rgb_to_yuv420");
}
