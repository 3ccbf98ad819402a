// One resident packed I420 frame -> the window a dataset evaluation needs (include/atmvfi.h, atmvfi_yuv420_window): the output of
// atmvfi_frame_u8_window on the frame atmvfi_yuv420_to_rgb would write, without that RGB frame ever existing.  The Xiph 2K / 4K
// evaluation reads its clips as 10-bit 4:2:0 Y4M this way (atm-vfi_amd/evaluate.py).  No new arithmetic: with q(Y, X) the clip8 RGB pixel
// of the WHOLE frame's decode (chroma neighbours clamp at the frame's edges, never at the window's),
//   mode 0: out(y, x) = q(y0 + y, x0 + x)
//   mode 1: out(y, x) = (q(y0 + 2y, x0 + 2x) + q(y0 + 2y, x0 + 2x + 1) + q(y0 + 2y + 1, x0 + 2x) + q(y0 + 2y + 1, x0 + 2x + 1) + 2) >> 2
//           per channel: four 8-bit pixels, then the area rule (the order of an rgb24 PNG followed by cv2.INTER_AREA)
// as fp32 planar [3,Hp,Wp] = out / 255 (the bits of the fp32 division) with replicate padding by clamping the output coordinate into
// the window, and / or uint8 [h,w,3] RGB un-padded.  Every decode helper is yuv_common.h's, so the bits are yuv.hip's by construction.
//
// A lane makes four horizontally adjacent pixels of the PADDED output, as in yuv.hip and frames.hip:
//   mode 0: on two output rows -- a 4 x 2 block of source luma, two to three chroma rows of four samples, a shared row loaded once;
//   mode 1: on one output row -- an 8 x 2 block of source luma (rows y0 + 2y and y0 + 2y + 1 lie on one chroma row r because y0 is
//           even; they filter with rows r - 1 and r + 1), so the plane stores stay 16 bytes wide; the three chroma rows are loaded
//           once, six samples wide, and both halves of the block decode from them.
//   aligned path (frame and uint8 pointers 4-byte, fp32 pointer 16-byte aligned; W, x0, w, Wp, pad_left multiples of 4): dword Y loads,
//           2-byte / dword chroma pairs, 16-byte plane stores, 12-byte RGB groups; a group lies wholly inside the window or wholly in
//           the padding, and a padding group decodes the nearest inside group and repeats its edge pixel.
//   general path: any geometry and alignment: one decode_pixel per source pixel, scalar stores, the same bits.
// Vector stores only, no atomics, nothing pre-zeroed: every output byte is written by exactly one lane.
#include "yuv_common.h"

namespace {

struct WinArgs : YuvSrc {
    int y0, x0, h, w;           // the window in OUTPUT pixels (mode 1 reads 2h x 2w source pixels)
    float* dst;
    int Hp, Wp, pad_top, pad_left;
    unsigned char* dst_u8;
    int groups;                 // ceil(Wp / 4)
    int rows;                   // lanes per column of groups: ceil(Hp / 2) in mode 0, Hp in mode 1
};

// one group of the aligned path -> the canvas and the uint8 window; (y, x) canvas coordinates, (wy, wx) window coordinates of its first pixel
__device__ __forceinline__ void store_group(const WinArgs& a, int y, int x, int wy, int wx, int q[4][3]) {
    const bool in = wx >= 0 && wx < a.w;
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
    if (a.dst_u8 && in && wy >= 0 && wy < a.h) {
        unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[(3 * i + c) >> 2] |= (unsigned)q[i][c] << (((3 * i + c) & 3) * 8);
        }
        *reinterpret_cast<U32x3*>(a.dst_u8 + ((long long)wy * a.w + wx) * 3) = U32x3{d[0], d[1], d[2]};
    }
}

// one pixel of the general path
__device__ __forceinline__ void store_pixel(const WinArgs& a, int y, int x, int wy, int wx, const int q[3]) {
    if (a.dst) {
        const long long plane = (long long)a.Hp * a.Wp;
        float* o = a.dst + (long long)y * a.Wp + x;
        o[0] = q255(q[0]);
        o[plane] = q255(q[1]);
        o[2 * plane] = q255(q[2]);
    }
    if (a.dst_u8 && wy >= 0 && wy < a.h && wx >= 0 && wx < a.w) {
        unsigned char* o = a.dst_u8 + ((long long)wy * a.w + wx) * 3;
        o[0] = (unsigned char)q[0];
        o[1] = (unsigned char)q[1];
        o[2] = (unsigned char)q[2];
    }
}

// mode 0: the decode kernel of yuv.hip with the frame coordinate moved by the window's origin
template <int DEPTH, bool ALIGNED, bool LEFT>
__global__ __launch_bounds__(256) void yuv420_window_crop_kernel(const WinArgs a) {
    const int total = a.rows * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int k = idx / a.groups, x = (idx - k * a.groups) * 4;
        const int wx = x - a.pad_left;
        if (ALIGNED) {
            const int gx = a.x0 + clampi(wx, 0, a.w - 4), q = gx >> 1;
            const int yA = 2 * k, yB = yA + 1;
            const int fyA = a.y0 + clampi(yA - a.pad_top, 0, a.h - 1), fyB = a.y0 + clampi(yB - a.pad_top, 0, a.h - 1);
            const int rA0 = fyA >> 1, rA1 = clampi(rA0 + ((fyA & 1) ? 1 : -1), 0, a.ch - 1);
            int uA0[4], uA1[4], vA0[4], vA1[4], px[4][3];
            load_seg<DEPTH, true>(a, a.uoff, rA0, q, uA0);
            load_seg<DEPTH, true>(a, a.voff, rA0, q, vA0);
            load_seg<DEPTH, true>(a, a.uoff, rA1, q, uA1);
            load_seg<DEPTH, true>(a, a.voff, rA1, q, vA1);
            decode4<DEPTH, LEFT>(a, fyA, gx, uA0, uA1, vA0, vA1, px);
            store_group(a, yA, x, yA - a.pad_top, wx, px);
            if (yB < a.Hp) {
                const int rB0 = fyB >> 1, rB1 = clampi(rB0 + ((fyB & 1) ? 1 : -1), 0, a.ch - 1);
                int uB0[4], uB1[4], vB0[4], vB1[4];
                // a chroma row both luma rows use is already here: inside the window one of row B's two rows always is
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
                decode4<DEPTH, LEFT>(a, fyB, gx, uB0, uB1, vB0, vB1, px);
                store_group(a, yB, x, yB - a.pad_top, wx, px);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = 2 * k + r, wy = y - a.pad_top;
                if (y >= a.Hp) break;
                const int fy = a.y0 + clampi(wy, 0, a.h - 1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (x + i >= a.Wp) break;
                    int q[3];
                    decode_pixel<DEPTH, LEFT>(a, fy, a.x0 + clampi(wx + i, 0, a.w - 1), q);
                    store_pixel(a, y, x + i, wy, wx + i, q);
                }
            }
        }
    }
}

// seg[k] = plane[r][clamp(q - 1 + k, 0, cw - 1)], k = 0..5: every chroma column that luma columns 2q .. 2q + 7 touch (q even, cw even, the
// columns q .. q + 3 inside the row: two naturally aligned pairs); seg + 2 is load_seg's segment of luma columns 2q + 4 .. 2q + 7
template <int DEPTH>
__device__ __forceinline__ void load_seg6(const YuvSrc& a, long long plane, int r, int q, int seg[6]) {
    const long long row = plane + (long long)r * a.cw;
    seg[0] = sample<DEPTH, true>(a.yuv, row + max(q - 1, 0));
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (DEPTH == 8) {
            const unsigned v = reinterpret_cast<const U16x1*>(a.yuv + row + q + 2 * p)->v;
            seg[1 + 2 * p] = (int)(v & 0xffu);
            seg[2 + 2 * p] = (int)(v >> 8);
        } else {
            const unsigned v = *reinterpret_cast<const unsigned*>(a.yuv + 2 * (row + q + 2 * p));
            seg[1 + 2 * p] = (int)(v & 0xffffu);
            seg[2 + 2 * p] = (int)(v >> 16);
        }
    }
    seg[5] = sample<DEPTH, true>(a.yuv, row + min(q + 4, a.cw - 1));
}

// mode 1: four output pixels of one output row from source rows fy (even) and fy + 1, columns gx .. gx + 7
template <int DEPTH, bool ALIGNED, bool LEFT>
__global__ __launch_bounds__(256) void yuv420_window_area_kernel(const WinArgs a) {
    const int total = a.rows * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        const int wy = y - a.pad_top, wx = x - a.pad_left;
        const int fy = a.y0 + 2 * clampi(wy, 0, a.h - 1);           // even: rows fy and fy + 1 share chroma row fy >> 1
        if (ALIGNED) {
            const int gx = a.x0 + 2 * clampi(wx, 0, a.w - 4);
            const int r = fy >> 1, rm = max(r - 1, 0), rp = min(r + 1, a.ch - 1);
            int px[4][3], u[3][6], v[3][6];         // the three chroma rows, six samples wide, loaded once for both halves
            load_seg6<DEPTH>(a, a.uoff, rm, gx >> 1, u[0]);
            load_seg6<DEPTH>(a, a.voff, rm, gx >> 1, v[0]);
            load_seg6<DEPTH>(a, a.uoff, r, gx >> 1, u[1]);
            load_seg6<DEPTH>(a, a.voff, r, gx >> 1, v[1]);
            load_seg6<DEPTH>(a, a.uoff, rp, gx >> 1, u[2]);
            load_seg6<DEPTH>(a, a.voff, rp, gx >> 1, v[2]);
#pragma unroll
            for (int half = 0; half < 2; ++half) {          // source columns gx + 4 half .. + 3 -> output pixels 2 half, 2 half + 1
                const int hx = gx + 4 * half, o = 2 * half;
                int top[4][3], bot[4][3];
                decode4<DEPTH, LEFT>(a, fy, hx, u[1] + o, u[0] + o, v[1] + o, v[0] + o, top);            // even row: (r, r - 1), weights (3, 1)
                decode4<DEPTH, LEFT>(a, fy + 1, hx, u[1] + o, u[2] + o, v[1] + o, v[2] + o, bot);        // odd row: (r, r + 1)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[2 * half + j][c] = (top[2 * j][c] + top[2 * j + 1][c] + bot[2 * j][c] + bot[2 * j + 1][c] + 2) >> 2;
            }
            store_group(a, y, x, wy, wx, px);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.Wp) break;
                const int fx = a.x0 + 2 * clampi(wx + i, 0, a.w - 1);
                int s[4][3], q[3];
                decode_pixel<DEPTH, LEFT>(a, fy, fx, s[0]);
                decode_pixel<DEPTH, LEFT>(a, fy, fx + 1, s[1]);
                decode_pixel<DEPTH, LEFT>(a, fy + 1, fx, s[2]);
                decode_pixel<DEPTH, LEFT>(a, fy + 1, fx + 1, s[3]);
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c] = (s[0][c] + s[1][c] + s[2][c] + s[3][c] + 2) >> 2;
                store_pixel(a, y, x + i, wy, wx + i, q);
            }
        }
    }
}

}  // namespace

extern "C" int atmvfi_yuv420_window(const void* yuv, int H, int W, int depth, int matrix, int full_range, int siting, int mode, int y0, int x0,
                                    int h, int w, float* dst, int Hp, int Wp, int pad_top, int pad_left, void* dst_u8, void* stream) {
    ATMVFI_REQUIRE(yuv, ATMVFI_EINVAL, "yuv420_window: null source");
    ATMVFI_REQUIRE(dst || dst_u8, ATMVFI_EINVAL, "yuv420_window: both outputs are null (give dst, dst_u8 or both)");
    if (const int rc = check_format("yuv420_window", H, W, matrix, full_range, siting)) return rc;
    ATMVFI_REQUIRE(depth == 8 || depth == 10, ATMVFI_EINVAL, "yuv420_window: depth must be 8 or 10 (got %d)", depth);
    ATMVFI_REQUIRE(!(depth == 10 && full_range), ATMVFI_EINVAL, "yuv420_window: 10-bit full range is not supported");
    ATMVFI_REQUIRE(mode == 0 || mode == 1, ATMVFI_EINVAL, "yuv420_window: unknown mode %d (0: crop, 1: area 2x)", mode);
    ATMVFI_REQUIRE(h > 0 && w > 0 && y0 >= 0 && x0 >= 0, ATMVFI_EINVAL, "yuv420_window: negative or zero size (window %d x %d at (%d, %d))", h, w,
                   y0, x0);
    const long long s = mode == 1 ? 2 : 1;
    ATMVFI_REQUIRE(y0 + s * h <= H && x0 + s * w <= W, ATMVFI_EINVAL,
                   "yuv420_window: window outside the frame (mode %d reads %lld x %lld source pixels at (%d, %d) of a %d x %d frame)", mode,
                   s * h, s * w, y0, x0, H, W);
    ATMVFI_REQUIRE(y0 % 2 == 0 && x0 % 2 == 0, ATMVFI_EINVAL, "yuv420_window: the window origin (%d, %d) must be even for 4:2:0 frames", y0, x0);
    if (dst) {
        ATMVFI_REQUIRE(aligned4(dst), ATMVFI_EINVAL, "yuv420_window: dst must be 4-byte aligned");
        ATMVFI_REQUIRE(pad_top >= 0 && pad_left >= 0 && (long long)h + pad_top <= Hp && (long long)w + pad_left <= Wp, ATMVFI_EINVAL,
                       "yuv420_window: canvas %d x %d is smaller than the window %d x %d plus padding (%d, %d)", Hp, Wp, h, w, pad_top, pad_left);
    } else {        // no canvas: the output geometry is the window's
        Hp = h;
        Wp = w;
        pad_top = pad_left = 0;
    }
    const int groups = (int)(((long long)Wp + 3) / 4), rows = mode == 1 ? Hp : (int)(((long long)Hp + 1) / 2);
    ATMVFI_REQUIRE((long long)rows * groups < (1ll << 30), ATMVFI_EINVAL, "yuv420_window: output of %d x %d is too large", Hp, Wp);
    const WinArgs a = {make_src(yuv, H, W, depth, matrix, full_range), y0, x0, h, w, dst, Hp, Wp, pad_top, pad_left, (unsigned char*)dst_u8,
                       groups, rows};
    // aligned path: Y groups are dwords, chroma pairs naturally aligned (cw even, group origins even), plane stores 16 bytes, RGB groups
    // three dwords; a group of four lies wholly inside the window or wholly in the padding
    const bool al = aligned4(yuv) && W % 4 == 0 && x0 % 4 == 0 && w % 4 == 0 && pad_left % 4 == 0 && Wp % 4 == 0 &&
                    (!dst || atmvfi::aligned16(dst)) && (!dst_u8 || aligned4(dst_u8));
    const long long blocks = ((long long)rows * groups + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    // the siting is a template parameter: the tap indices and weights of the chroma filter are constants of the instance
#define ATMVFI_YUV_WINDOW(KERNEL, DEPTH, AL)                                                                           \
    do {                                                                                                               \
        if (siting) hipLaunchKernelGGL((KERNEL<DEPTH, AL, true>), grid, block, 0, st, a);                              \
        else hipLaunchKernelGGL((KERNEL<DEPTH, AL, false>), grid, block, 0, st, a);                                    \
    } while (0)
#define ATMVFI_YUV_WINDOW_MODE(KERNEL)                                                                                 \
    do {                                                                                                               \
        if (depth == 8) {                                                                                              \
            if (al) ATMVFI_YUV_WINDOW(KERNEL, 8, true);                                                                \
            else ATMVFI_YUV_WINDOW(KERNEL, 8, false);                                                                  \
        } else {                                                                                                       \
            if (al) ATMVFI_YUV_WINDOW(KERNEL, 10, true);                                                               \
            else ATMVFI_YUV_WINDOW(KERNEL, 10, false);                                                                 \
        }                                                                                                              \
    } while (0)
    if (mode == 0) ATMVFI_YUV_WINDOW_MODE(yuv420_window_crop_kernel);
    else ATMVFI_YUV_WINDOW_MODE(yuv420_window_area_kernel);
#undef ATMVFI_YUV_WINDOW_MODE
#undef ATMVFI_YUV_WINDOW
    return atmvfi::check_launch("yuv420_window");
}
