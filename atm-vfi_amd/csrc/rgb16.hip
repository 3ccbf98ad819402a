// Deep RGB frames (10 / 12 / 16 bit) <-> the network's fp32 planar canvas (include/atmvfi.h, atmvfi_rgb16_decode / atmvfi_rgb16_encode;
// atm-vfi_amd/pixfmt.py DeepRGB holds the layouts, atm-vfi_amd/rgb16.py the host twins, tests/cpu_rgb16.py the per-sample model).  Nothing of
// the reference.  Samples are little-endian uint16, LSB-aligned, top = 2^depth - 1:
//   layout 0 rgb48 : interleaved R G B, the bytes of a uint16 [H,W,3] array
//   layout 1 bgr48 : interleaved B G R
//   layout 2 gbrp  : three tight planes [H,W] in the order G, B, R
//   decode  q' = min(q, top); fp32 planar RGB [3,Hp,Wp] = q' / top with the bits of the fp32 division (frame_u8_to_f32's pixel with top in
//           place of 255), the window (y0, x0, h, w) at (pad_top, pad_left), replicate padding of the window's own edge pixels; and / or
//           the probe picture uint8 [h,w,3] RGB = q' >> (depth - 8)
//   encode  p = clip(rint(fl32(x * top)), 0, top), half to even (frame_f32_to_u8's pixel with top in place of 255), in the layout's order
//
// Byte-bound: decode reads 6 and writes 12 (+ 3) bytes per pixel, encode reads 12 and writes 6.  A lane owns four adjacent pixels of a row
// (decode: of the PADDED canvas, as frames.hip, so the padding is written by the lanes that own it: one launch).
//   aligned path: the fp32 side is one 16-byte access per plane; the four pixels of an interleaved frame are 24 contiguous bytes moved as
//                 three 8-byte accesses, those of a gbrp frame 8 bytes per plane; the probe's four pixels are three dwords.  Needs an 8-byte
//                 aligned frame, W % 4 == 0 (a window: x0 % 4 == 0, w % 4 == 0), a 16-byte aligned canvas with Wp % 4 == 0 and
//                 pad_left % 4 == 0, a 4-byte aligned probe picture.  A group of four lies wholly inside the window or wholly in the
//                 padding; a padding group loads the nearest inside group and repeats its edge pixel.
//   general path: any geometry, sample-aligned pointers: 2-byte accesses of the frame, scalar accesses of the canvas, the same arithmetic.
// The component permutation of bgr48 / gbrp happens in registers.  Grid-stride (grid_for), 256 threads, every output byte written by
// exactly one lane, vector stores only, no atomics, nothing pre-zeroed, no LDS.
#include "common.h"

namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
struct alignas(4) U32x3 {
    unsigned a, b, c;
};

enum { RGB48 = 0, BGR48 = 1, GBRP = 2 };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the RGB channel held by memory slot (interleaved) or plane (gbrp) s of a layout
template <int LAYOUT>
__device__ __forceinline__ constexpr int channel_of(int s) {
    return LAYOUT == RGB48 ? s : LAYOUT == BGR48 ? 2 - s : (s == 0 ? 1 : s == 1 ? 2 : 0);
}

struct DecodeArgs {
    const unsigned short* src;
    int H, W;
    int y0, x0, h, w;
    float* dst;
    int Hp, Wp, pad_top, pad_left;      // (without dst: the window itself, no padding)
    unsigned char* dst_u8;
    int groups;                         // ceil(Wp / 4)
    int top, shift;                     // 2^depth - 1, depth - 8
    float topf, rcp;                    // (float)top, fl32(1 / top)
};

// q / top for an integer q in 0..top with the bits of the fp32 division: q * r with r = fl(1 / top), then one correction step in fused
// multiply-adds (yuv_common.h q255 / q1023; equal to the division for every code of depths 10, 12 and 16: tests/test_rgb16_cpu.py
// checks all of them in exact rational arithmetic)
__device__ __forceinline__ float unit_of(int q, float topf, float rcp) {
    const float f = (float)q;
    const float y = f * rcp;
    return __fmaf_rn(__fmaf_rn(-topf, y, f), rcp, y);
}

template <int LAYOUT, bool ALIGNED>
__global__ __launch_bounds__(256) void rgb16_decode_kernel(const DecodeArgs a) {
    const long long plane = (long long)a.Hp * a.Wp, frame = (long long)a.H * a.W;
    const int total = a.Hp * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        const int wy = y - a.pad_top, wx = x - a.pad_left;        // window coordinates of the group's first pixel; outside = padding
        const int oy = clampi(wy, 0, a.h - 1);
        const bool row_in = wy >= 0 && wy < a.h;
        const long long row = (long long)(a.y0 + oy) * a.W + a.x0;
        if (ALIGNED) {
            int q[4][3];        // [pixel][R, G, B]
            const int ox = clampi(wx, 0, a.w - 4);
            if (LAYOUT == GBRP) {
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const u32x2 v = *reinterpret_cast<const u32x2*>(a.src + s * frame + row + ox);
                    const int c = channel_of<LAYOUT>(s);
                    q[0][c] = (int)(v[0] & 0xffffu), q[1][c] = (int)(v[0] >> 16), q[2][c] = (int)(v[1] & 0xffffu), q[3][c] = (int)(v[1] >> 16);
                }
            } else {
                const u32x2* p = reinterpret_cast<const u32x2*>(a.src + (row + ox) * 3);
                const u32x2 v0 = p[0], v1 = p[1], v2 = p[2];
                const unsigned d[6] = {v0[0], v0[1], v1[0], v1[1], v2[0], v2[1]};
#pragma unroll
                for (int k = 0; k < 12; ++k) q[k / 3][channel_of<LAYOUT>(k % 3)] = (int)((d[k >> 1] >> ((k & 1) * 16)) & 0xffffu);
            }
            const bool in = wx >= 0 && wx < a.w;
            if (!in) {          // left padding repeats the first pixel of the first group, right padding the last of the last
#pragma unroll
                for (int c = 0; c < 3; ++c) q[0][c] = q[1][c] = q[2][c] = q[3][c] = wx < 0 ? q[0][c] : q[3][c];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) q[i][c] = min(q[i][c], a.top);
            if (a.dst) {
                float* o = a.dst + (long long)y * a.Wp + x;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    *reinterpret_cast<f32x4*>(o + c * plane) = (f32x4){unit_of(q[0][c], a.topf, a.rcp), unit_of(q[1][c], a.topf, a.rcp),
                                                                       unit_of(q[2][c], a.topf, a.rcp), unit_of(q[3][c], a.topf, a.rcp)};
            }
            if (a.dst_u8 && in && row_in) {
                unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[(3 * i + c) >> 2] |= (unsigned)(q[i][c] >> a.shift) << (((3 * i + c) & 3) * 8);
                }
                *reinterpret_cast<U32x3*>(a.dst_u8 + ((long long)wy * a.w + wx) * 3) = U32x3{d[0], d[1], d[2]};
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.Wp) break;
                const int ox = clampi(wx + i, 0, a.w - 1);
                int q[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const unsigned short v = LAYOUT == GBRP ? a.src[s * frame + row + ox] : a.src[(row + ox) * 3 + s];
                    q[channel_of<LAYOUT>(s)] = min((int)v, a.top);
                }
                if (a.dst) {
                    float* o = a.dst + (long long)y * a.Wp + x + i;
                    o[0] = unit_of(q[0], a.topf, a.rcp);
                    o[plane] = unit_of(q[1], a.topf, a.rcp);
                    o[2 * plane] = unit_of(q[2], a.topf, a.rcp);
                }
                if (a.dst_u8 && row_in && wx + i >= 0 && wx + i < a.w) {
                    unsigned char* o = a.dst_u8 + ((long long)wy * a.w + wx + i) * 3;
                    o[0] = (unsigned char)(q[0] >> a.shift);
                    o[1] = (unsigned char)(q[1] >> a.shift);
                    o[2] = (unsigned char)(q[2] >> a.shift);
                }
            }
        }
    }
}

struct EncodeArgs {
    const float* src;
    int Hp, Wp, pad_top, pad_left;
    unsigned short* dst;
    int H, W;
    int groups;                         // ceil(W / 4)
    int top;
    float topf;
};

__device__ __forceinline__ unsigned pixel_of(float x, float topf, int top) {
    const int q = __float2int_rn(x * topf);        // rint: half to even, as np.rint (frame_f32_to_u8); the conversion saturates
    return (unsigned)(q < 0 ? 0 : (q > top ? top : q));
}

template <int LAYOUT, bool ALIGNED>
__global__ __launch_bounds__(256) void rgb16_encode_kernel(const EncodeArgs a) {
    const long long plane = (long long)a.Hp * a.Wp, frame = (long long)a.H * a.W;
    const int total = a.H * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        const float* s = a.src + (long long)(y + a.pad_top) * a.Wp + (x + a.pad_left);
        const long long row = (long long)y * a.W + x;
        if (ALIGNED) {
            unsigned p[4][3];       // [pixel][R, G, B]
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(s + c * plane);
                p[0][c] = pixel_of(v.x, a.topf, a.top), p[1][c] = pixel_of(v.y, a.topf, a.top);
                p[2][c] = pixel_of(v.z, a.topf, a.top), p[3][c] = pixel_of(v.w, a.topf, a.top);
            }
            if (LAYOUT == GBRP) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int c = channel_of<LAYOUT>(k);
                    *reinterpret_cast<u32x2*>(a.dst + k * frame + row) = u32x2{p[0][c] | p[1][c] << 16, p[2][c] | p[3][c] << 16};
                }
            } else {
                unsigned d[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 12; ++k) d[k >> 1] |= p[k / 3][channel_of<LAYOUT>(k % 3)] << ((k & 1) * 16);
                u32x2* o = reinterpret_cast<u32x2*>(a.dst + row * 3);
                o[0] = u32x2{d[0], d[1]};
                o[1] = u32x2{d[2], d[3]};
                o[2] = u32x2{d[4], d[5]};
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.W) break;
                unsigned p[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = pixel_of(s[c * plane + i], a.topf, a.top);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const unsigned short v = (unsigned short)p[channel_of<LAYOUT>(k)];
                    if (LAYOUT == GBRP) a.dst[k * frame + row + i] = v;
                    else a.dst[(row + i) * 3 + k] = v;
                }
            }
        }
    }
}

inline bool aligned_to(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) == 0; }

const char* const kLayoutNames[3] = {"rgb48", "bgr48", "gbrp"};

template <template <int, bool> class Launch, typename Args>
void dispatch(int layout, bool aligned, dim3 grid, hipStream_t st, const Args& a) {
    switch (layout * 2 + (aligned ? 1 : 0)) {
        case 0: Launch<RGB48, false>::go(grid, st, a); break;
        case 1: Launch<RGB48, true>::go(grid, st, a); break;
        case 2: Launch<BGR48, false>::go(grid, st, a); break;
        case 3: Launch<BGR48, true>::go(grid, st, a); break;
        case 4: Launch<GBRP, false>::go(grid, st, a); break;
        default: Launch<GBRP, true>::go(grid, st, a); break;
    }
}
template <int LAYOUT, bool ALIGNED>
struct LaunchDecode {
    static void go(dim3 grid, hipStream_t st, const DecodeArgs& a) {
        hipLaunchKernelGGL((rgb16_decode_kernel<LAYOUT, ALIGNED>), grid, dim3(256), 0, st, a);
    }
};
template <int LAYOUT, bool ALIGNED>
struct LaunchEncode {
    static void go(dim3 grid, hipStream_t st, const EncodeArgs& a) {
        hipLaunchKernelGGL((rgb16_encode_kernel<LAYOUT, ALIGNED>), grid, dim3(256), 0, st, a);
    }
};

}  // namespace

extern "C" int atmvfi_rgb16_decode(const void* src, int H, int W, int depth, int layout, int y0, int x0, int h, int w, float* dst, int Hp,
                                    int Wp, int pad_top, int pad_left, void* dst_u8, void* stream) {
    ATMVFI_REQUIRE(src, ATMVFI_EINVAL, "rgb16_decode: null source");
    ATMVFI_REQUIRE(dst || dst_u8, ATMVFI_EINVAL, "rgb16_decode: both outputs are null (give dst, dst_u8 or both)");
    ATMVFI_REQUIRE(depth == 10 || depth == 12 || depth == 16, ATMVFI_EINVAL, "rgb16_decode: depth must be 10, 12 or 16 (got %d)", depth);
    ATMVFI_REQUIRE(layout >= 0 && layout <= 2, ATMVFI_EINVAL, "rgb16_decode: unknown layout %d (0: rgb48, 1: bgr48, 2: gbrp)", layout);
    ATMVFI_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0 && y0 >= 0 && x0 >= 0, ATMVFI_EINVAL,
                   "rgb16_decode: negative or zero size (H %d W %d, window %d x %d at (%d, %d))", H, W, h, w, y0, x0);
    ATMVFI_REQUIRE((long long)y0 + h <= H && (long long)x0 + w <= W, ATMVFI_EINVAL,
                   "rgb16_decode: window %d x %d at (%d, %d) outside the %d x %d frame", h, w, y0, x0, H, W);
    if (dst) {
        ATMVFI_REQUIRE(Hp > 0 && Wp > 0 && pad_top >= 0 && pad_left >= 0, ATMVFI_EINVAL, "rgb16_decode: bad canvas (Hp %d Wp %d, pad %d %d)", Hp,
                       Wp, pad_top, pad_left);
        ATMVFI_REQUIRE((long long)h + pad_top <= Hp, ATMVFI_EINVAL, "rgb16_decode: Hp %d < h %d + pad_top %d", Hp, h, pad_top);
        ATMVFI_REQUIRE((long long)w + pad_left <= Wp, ATMVFI_EINVAL, "rgb16_decode: Wp %d < w %d + pad_left %d", Wp, w, pad_left);
    } else {        // the probe picture alone: the window itself
        Hp = h, Wp = w, pad_top = pad_left = 0;
    }
    ATMVFI_REQUIRE(aligned_to(src, 2) && aligned_to(dst, 4), ATMVFI_EINVAL,
                   "rgb16_decode: a %s frame must be 2-byte aligned and the canvas 4-byte aligned (src %p, dst %p)", kLayoutNames[layout], src, (void*)dst);
    const int groups = (int)(((long long)Wp + 3) / 4);
    ATMVFI_REQUIRE((long long)Hp * groups < (1ll << 30) && (long long)H * W < (1ll << 40), ATMVFI_EINVAL,
                   "rgb16_decode: a canvas of %d x %d (frame %d x %d) is too large", Hp, Wp, H, W);
    const bool al = aligned_to(src, 8) && W % 4 == 0 && x0 % 4 == 0 && w % 4 == 0 && pad_left % 4 == 0 && Wp % 4 == 0 &&
                    (!dst || atmvfi::aligned16(dst)) && (!dst_u8 || aligned_to(dst_u8, 4));
    const int top = (1 << depth) - 1;
    const DecodeArgs a = {(const unsigned short*)src, H, W, y0, x0, h, w, dst, Hp, Wp, pad_top, pad_left, (unsigned char*)dst_u8, groups, top,
                          depth - 8, (float)top, 1.0f / (float)top};
    dispatch<LaunchDecode>(layout, al, dim3(grid_for((long long)Hp * groups)), (hipStream_t)stream, a);
    return atmvfi::check_launch("rgb16_decode");
}

extern "C" int atmvfi_rgb16_encode(const float* src, int Hp, int Wp, int pad_top, int pad_left, void* dst, int H, int W, int depth,
                                    int layout, void* stream) {
    ATMVFI_REQUIRE(src && dst, ATMVFI_EINVAL, "rgb16_encode: null pointer (src %p, dst %p)", (const void*)src, dst);
    ATMVFI_REQUIRE(depth == 10 || depth == 12 || depth == 16, ATMVFI_EINVAL, "rgb16_encode: depth must be 10, 12 or 16 (got %d)", depth);
    ATMVFI_REQUIRE(layout >= 0 && layout <= 2, ATMVFI_EINVAL, "rgb16_encode: unknown layout %d (0: rgb48, 1: bgr48, 2: gbrp)", layout);
    ATMVFI_REQUIRE(H > 0 && W > 0 && Hp > 0 && Wp > 0 && pad_top >= 0 && pad_left >= 0 && (long long)H + pad_top <= Hp && (long long)W + pad_left <= Wp,
                   ATMVFI_EINVAL, "rgb16_encode: bad geometry (Hp %d Wp %d -> H %d W %d, pad %d %d)", Hp, Wp, H, W, pad_top, pad_left);
    ATMVFI_REQUIRE(aligned_to(dst, 2) && aligned_to(src, 4), ATMVFI_EINVAL,
                   "rgb16_encode: a %s frame must be 2-byte aligned and the canvas 4-byte aligned (src %p, dst %p)", kLayoutNames[layout], (const void*)src, dst);
    const int groups = (int)(((long long)W + 3) / 4);
    ATMVFI_REQUIRE((long long)H * groups < (1ll << 30), ATMVFI_EINVAL, "rgb16_encode: a frame of %d x %d is too large", H, W);
    const bool al = aligned_to(dst, 8) && W % 4 == 0 && atmvfi::aligned16(src) && Wp % 4 == 0 && pad_left % 4 == 0;
    const int top = (1 << depth) - 1;
    const EncodeArgs a = {src, Hp, Wp, pad_top, pad_left, (unsigned short*)dst, H, W, groups, top, (float)top};
    dispatch<LaunchEncode>(layout, al, dim3(grid_for((long long)H * groups)), (hipStream_t)stream, a);
    return atmvfi::check_launch("rgb16_encode");
}
