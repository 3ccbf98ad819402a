// Frame preparation for the dataset evaluations at 2K / 4K (benchmark/test_xiph.py of the reference): one resident uint8 [H,W,3]
// frame -> any number of network inputs and ground truths, without going back to the host (include/atmvfi.h, atmvfi_frame_u8_window).
//   mode 0: an h x w window of the frame at (y0, x0)
//   mode 1: the 2x area reduction of the 2h x 2w window at (y0, x0): (a + b + c + d + 2) >> 2 per channel, cv2.INTER_AREA for uint8
//           at an exact scale of 2 (ties round up)
// Outputs, either or both: fp32 planar RGB [3,Hp,Wp] = q / 255 (a true fp32 division, as frame_u8_to_f32) with replicate padding, the
// window sitting at (pad_top, pad_left); uint8 [h,w,3] RGB, the same integer pixels un-padded (what atmvfi_ssim_psnr reads in place).
//
// Bandwidth-bound; a 4096x2160 frame is 26.5 MB in (mode 1) and 26.7 + 6.6 MB out.  One lane makes 4 horizontally adjacent pixels of the
// PADDED output: three 16-byte plane stores, and 12 contiguous bytes of the uint8 output.  Padding comes from clamping the output
// coordinate, never from a second pass.
//   aligned path: dword loads (12 contiguous source bytes per lane in mode 0, 24 on each of two rows in mode 1), float4 / dword stores.
//                 A group of four lies wholly inside the window or wholly in the padding (pad_left % 4 == 0, w % 4 == 0); a padding
//                 group loads the nearest inside group and repeats its edge pixel, so every lane of a wave runs the same loads.
//   general path: any x0, w, Wp, pad_left and pointer alignment: byte loads, scalar stores, the same arithmetic.
// Integer work and one division: bit-exact against the numpy model (tests/cpu_frames.py) by construction.
#include "common.h"

namespace {

struct alignas(4) U32x3 {
    unsigned a, b, c;
};
struct alignas(4) U32x6 {
    unsigned v[6];
};

__device__ __forceinline__ int byte_of(const unsigned* d, int k) { return (int)((d[k >> 2] >> ((k & 3) * 8)) & 0xffu); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct FrameArgs {
    const unsigned char* src;
    long long pitch;        // 3 * W
    int y0, x0, h, w;
    float* dst;
    int Hp, Wp, pad_top, pad_left;
    unsigned char* dst_u8;
    int groups;             // ceil(Wp / 4)
};

// q[i][c]: output pixel i of the group, channel c in source order (the kernel swaps 0 and 2 for a BGR source)
template <int MODE>
__device__ __forceinline__ void load_group_aligned(const FrameArgs& a, int oy, int ox, int q[4][3]) {
    if (MODE == 0) {
        const U32x3 r = *reinterpret_cast<const U32x3*>(a.src + (long long)(a.y0 + oy) * a.pitch + (long long)(a.x0 + ox) * 3);
        const unsigned d[3] = {r.a, r.b, r.c};
#pragma unroll
        for (int k = 0; k < 12; ++k) q[k / 3][k % 3] = byte_of(d, k);
    } else {
        const unsigned char* p = a.src + (long long)(a.y0 + 2 * oy) * a.pitch + (long long)(a.x0 + 2 * ox) * 3;
        const U32x6 r0 = *reinterpret_cast<const U32x6*>(p);
        const U32x6 r1 = *reinterpret_cast<const U32x6*>(p + a.pitch);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                q[i][c] = (byte_of(r0.v, 6 * i + c) + byte_of(r0.v, 6 * i + 3 + c) + byte_of(r1.v, 6 * i + c) +
                           byte_of(r1.v, 6 * i + 3 + c) + 2) >> 2;
    }
}

template <int MODE>
__device__ __forceinline__ void load_pixel(const FrameArgs& a, int oy, int ox, int q[3]) {
    if (MODE == 0) {
        const unsigned char* p = a.src + (long long)(a.y0 + oy) * a.pitch + (long long)(a.x0 + ox) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = p[c];
    } else {
        const unsigned char* p = a.src + (long long)(a.y0 + 2 * oy) * a.pitch + (long long)(a.x0 + 2 * ox) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = ((int)p[c] + (int)p[3 + c] + (int)p[a.pitch + c] + (int)p[a.pitch + 3 + c] + 2) >> 2;
    }
}

template <int MODE, bool ALIGNED>
__global__ __launch_bounds__(256) void frame_u8_window_kernel(const FrameArgs a, const int bgr) {
    const long long plane = (long long)a.Hp * a.Wp;
    const int total = a.Hp * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        const int wy = y - a.pad_top, wx = x - a.pad_left;        // window coordinates of the group's first pixel; outside = padding
        const int oy = clampi(wy, 0, a.h - 1);
        const bool row_in = wy >= 0 && wy < a.h;
        if (ALIGNED) {
            int q[4][3];
            load_group_aligned<MODE>(a, oy, clampi(wx, 0, a.w - 4), q);
            const bool in = wx >= 0 && wx < a.w;
            if (!in) {          // left padding repeats the first pixel of the first group, right padding the last of the last
#pragma unroll
                for (int c = 0; c < 3; ++c) q[0][c] = q[1][c] = q[2][c] = q[3][c] = wx < 0 ? q[0][c] : q[3][c];
            }
            if (bgr) {          // (selects, not an index computed at run time: the pixels stay in registers)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int t = q[i][0];
                    q[i][0] = q[i][2];
                    q[i][2] = t;
                }
            }
            if (a.dst) {
                float* o = a.dst + (long long)y * a.Wp + x;
                *reinterpret_cast<f32x4*>(o) = (f32x4){(float)q[0][0] / 255.0f, (float)q[1][0] / 255.0f, (float)q[2][0] / 255.0f, (float)q[3][0] / 255.0f};
                *reinterpret_cast<f32x4*>(o + plane) = (f32x4){(float)q[0][1] / 255.0f, (float)q[1][1] / 255.0f, (float)q[2][1] / 255.0f, (float)q[3][1] / 255.0f};
                *reinterpret_cast<f32x4*>(o + 2 * plane) = (f32x4){(float)q[0][2] / 255.0f, (float)q[1][2] / 255.0f, (float)q[2][2] / 255.0f, (float)q[3][2] / 255.0f};
            }
            if (a.dst_u8 && in && row_in) {
                unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[(3 * i + c) >> 2] |= (unsigned)q[i][c] << (((3 * i + c) & 3) * 8);
                }
                *reinterpret_cast<U32x3*>(a.dst_u8 + ((long long)wy * a.w + wx) * 3) = U32x3{d[0], d[1], d[2]};
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.Wp) break;
                int q[3];
                load_pixel<MODE>(a, oy, clampi(wx + i, 0, a.w - 1), q);
                if (bgr) {
                    const int t = q[0];
                    q[0] = q[2];
                    q[2] = t;
                }
                if (a.dst) {
                    float* o = a.dst + (long long)y * a.Wp + x + i;
                    o[0] = (float)q[0] / 255.0f;
                    o[plane] = (float)q[1] / 255.0f;
                    o[2 * plane] = (float)q[2] / 255.0f;
                }
                if (a.dst_u8 && row_in && wx + i >= 0 && wx + i < a.w) {
                    unsigned char* o = a.dst_u8 + ((long long)wy * a.w + wx + i) * 3;
                    o[0] = (unsigned char)q[0];
                    o[1] = (unsigned char)q[1];
                    o[2] = (unsigned char)q[2];
                }
            }
        }
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int atmvfi_frame_u8_window(const void* src, int H, int W, int bgr, int mode, int y0, int x0, int h, int w, float* dst, int Hp,
                                       int Wp, int pad_top, int pad_left, void* dst_u8, void* stream) {
    ATMVFI_REQUIRE(src, ATMVFI_EINVAL, "frame_u8_window: null source");
    ATMVFI_REQUIRE(dst || dst_u8, ATMVFI_EINVAL, "frame_u8_window: both outputs are null (give dst, dst_u8 or both)");
    ATMVFI_REQUIRE(mode == 0 || mode == 1, ATMVFI_EINVAL, "frame_u8_window: unknown mode %d (0: crop, 1: area 2x)", mode);
    ATMVFI_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0 && y0 >= 0 && x0 >= 0 && Hp > 0 && Wp > 0 && pad_top >= 0 && pad_left >= 0,
                   ATMVFI_EINVAL, "frame_u8_window: negative or zero size (H %d W %d, window %d x %d at (%d, %d), Hp %d Wp %d, pad %d %d)", H,
                   W, h, w, y0, x0, Hp, Wp, pad_top, pad_left);
    const long long s = mode == 1 ? 2 : 1;
    ATMVFI_REQUIRE(y0 + s * h <= H && x0 + s * w <= W, ATMVFI_EINVAL,
                   "frame_u8_window: window outside the frame (mode %d reads %lld x %lld source pixels at (%d, %d) of a %d x %d frame)", mode,
                   s * h, s * w, y0, x0, H, W);
    ATMVFI_REQUIRE((long long)h + pad_top <= Hp, ATMVFI_EINVAL, "frame_u8_window: Hp %d < h %d + pad_top %d", Hp, h, pad_top);
    ATMVFI_REQUIRE((long long)w + pad_left <= Wp, ATMVFI_EINVAL, "frame_u8_window: Wp %d < w %d + pad_left %d", Wp, w, pad_left);
    const int groups = (int)(((long long)Wp + 3) / 4);
    ATMVFI_REQUIRE((long long)Hp * groups < (1ll << 30), ATMVFI_EINVAL, "frame_u8_window: output of %d x %d is too large", Hp, Wp);
    // aligned path: every load a dword, every plane store 16 bytes, every uint8 store a dword; groups never straddle the window's edge
    const bool al = aligned4(src) && W % 4 == 0 && x0 % 4 == 0 && w % 4 == 0 && pad_left % 4 == 0 && Wp % 4 == 0 &&
                    (!dst || atmvfi::aligned16(dst)) && (!dst_u8 || aligned4(dst_u8));
    const FrameArgs a = {(const unsigned char*)src, 3ll * W, y0, x0, h, w, dst, Hp, Wp, pad_top, pad_left, (unsigned char*)dst_u8, groups};
    const long long blocks = ((long long)Hp * groups + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (mode == 0) {
        if (al) hipLaunchKernelGGL((frame_u8_window_kernel<0, true>), grid, block, 0, st, a, bgr ? 1 : 0);
        else hipLaunchKernelGGL((frame_u8_window_kernel<0, false>), grid, block, 0, st, a, bgr ? 1 : 0);
    } else {
        if (al) hipLaunchKernelGGL((frame_u8_window_kernel<1, true>), grid, block, 0, st, a, bgr ? 1 : 0);
        else hipLaunchKernelGGL((frame_u8_window_kernel<1, false>), grid, block, 0, st, a, bgr ? 1 : 0);
    }
    return atmvfi::check_launch("frame_u8_window");
}
