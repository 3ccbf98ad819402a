// YUV 4:2:0 (and planar 4:2:2 / 4:4:4) -> RGB: atmvfi_yuv_decode of include/atmvfi.h, one kernel family behind one checked host path
// (below the kernels).  yuv_common.h holds the definition and every helper; yuv_encode.hip is the other direction.  The frame
// descriptor (atmvfi_yuv_desc) and the call's keep_depth / mode select what runs:
//   the whole frame, or a window of it -> fp32 planar [3,Hp,Wp] = q / 255 and / or uint8 [h,w,3] (RGB or BGR)
//   keep_depth (10 bit)       the depth kept -> fp32 planar = q / 1023
//   chroma / msb / strides    a decoder's surface (NV12 / NV21 / P010, planar; any pitch and chroma offset) -> either pixel of the two
//                             above: the same walker, instances with interleaved chroma and / or msb samples
//   subsampling 1 / 2         planar 4:2:2 / 4:4:4 frames, instances with SUB = 1 / 2.  On the aligned
//                             path 4:2:2 loads ONE chroma row per luma row (two per lane, no vertical mix), 4:4:4 loads U and V of a
//                             group as it loads Y (a dword, or 8 bytes at 10 bit)
//   mode                      the window a dataset evaluation needs (atm-vfi_amd/evaluate.py reads the Xiph 2K / 4K clips as 10-bit Y4M this
//                             way): the output of atmvfi_frame_u8_window on the frame the whole-frame decode would write, without that RGB
//                             frame ever existing.  With q(Y, X) the RGB pixel 0..255 of the WHOLE frame's decode,
//                               mode 0: out(y, x) = q(y0 + y, x0 + x) -- the whole-frame decode is this with the window set to the frame
//                               mode 1: out(y, x) = (q(y0 + 2y, x0 + 2x) + q(y0 + 2y, x0 + 2x + 1) + q(y0 + 2y + 1, x0 + 2x)
//                                       + q(y0 + 2y + 1, x0 + 2x + 1) + 2) >> 2 per channel: four 8-bit pixels, then the area rule (the
//                                       order of an rgb24 PNG followed by cv2.INTER_AREA)
//
// Bandwidth-bound: 1.5 or 3 B/px in and 12 out to fp32.  A lane makes four horizontally adjacent pixels of the PADDED output (padding
// comes from clamping the output coordinate into the window, as in frames.hip):
//   crop (mode 0): on two output rows -- a 4 x 2 block of source luma.  The two rows need at most three chroma
//           rows, four samples wide (columns q - 1 .. q + 2 of the group, clamped): a row that both luma rows use is loaded once.
//           Chroma is read straight from global memory: neighbouring lanes and rows re-read the same few bytes, which the vector L1
//           serves; the HBM traffic is the frame, once.
//   area (mode 1): on one output row -- an 8 x 2 block of source luma (rows y0 + 2y and y0 + 2y + 1 lie on one chroma row r because y0
//           is even; they filter with rows r - 1 and r + 1), so the plane stores stay 16 bytes wide; the three chroma rows are loaded
//           once, six samples wide, and both halves of the block decode from them.
//   aligned path (frame and uint8 pointers 4-byte, fp32 pointer 16-byte aligned; W, x0, w, Wp, pad_left multiples of 4): dword or 8-byte
//           Y loads, 2-byte / dword chroma pairs, 16-byte plane stores, 12-byte RGB groups; a group lies wholly inside the window or
//           wholly in the padding, and a padding group decodes the nearest inside group and repeats its edge pixel.
//           A surface also needs a pitch that is a multiple of 4 bytes and naturally aligned chroma (layout_aligned); its interleaved
//           chroma row is loaded ONCE for both planes: the centre pair-of-pairs as a dword or 8 bytes, each outer column as 2 or 4
//           bytes -- three loads per chroma row where two planes take six (load_row).
//   general path: any geometry and alignment: one decode_pixel per source pixel, scalar stores, the same integer arithmetic, the same bits.
// Vector stores only, no atomics, nothing pre-zeroed: every output byte is written by exactly one lane.
#include "yuv_common.h"

namespace {

struct DecOut {
    int y0, x0, h, w;           // the window in OUTPUT pixels (mode 1 reads 2h x 2w source pixels)
    float* dst;
    int Hp, Wp, pad_top, pad_left;
    unsigned char* dst_u8;      // (TOP == 255 only)
    int bgr;
    int groups;                 // ceil(Wp / 4)
    int rows;                   // lanes per column of groups: ceil(Hp / 2) for the crop, Hp in mode 1
};
struct DecArgs : YuvSrc, DecOut {};     // (yuv_common.h: the frame, its planes and the pixel)

// The sink, TOP = 255: the fp32 canvas via q255 and / or the uint8 window, RGB or BGR; TOP = 1023: the fp32 canvas via q1023.
// one group of the aligned path; (y, x) canvas coordinates, (wy, wx) window coordinates of its first pixel
template <int TOP>
__device__ __forceinline__ void store_group(const DecArgs& a, int y, int x, int wy, int wx, int q[4][3]) {
    const bool in = wx >= 0 && wx < a.w;
    if (!in) {          // left padding repeats the first pixel of the first group, right padding the last of the last
#pragma unroll
        for (int c = 0; c < 3; ++c) q[0][c] = q[1][c] = q[2][c] = q[3][c] = wx < 0 ? q[0][c] : q[3][c];
    }
    if (TOP != 255 || a.dst) {
        const long long plane = (long long)a.Hp * a.Wp;
        float* o = a.dst + (long long)y * a.Wp + x;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<f32x4*>(o + c * plane) = (f32x4){unit<TOP>(q[0][c]), unit<TOP>(q[1][c]), unit<TOP>(q[2][c]), unit<TOP>(q[3][c])};
    }
    if (TOP == 255 && a.dst_u8 && in && wy >= 0 && wy < a.h) {
        unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int v = a.bgr ? q[i][2 - c] : q[i][c];
                d[(3 * i + c) >> 2] |= (unsigned)v << (((3 * i + c) & 3) * 8);
            }
        }
        *reinterpret_cast<U32x3*>(a.dst_u8 + ((long long)wy * a.w + wx) * 3) = U32x3{d[0], d[1], d[2]};
    }
}

// one pixel of the general path
template <int TOP>
__device__ __forceinline__ void store_pixel(const DecArgs& a, int y, int x, int wy, int wx, const int q[3]) {
    if (TOP != 255 || a.dst) {
        const long long plane = (long long)a.Hp * a.Wp;
        float* o = a.dst + (long long)y * a.Wp + x;
        o[0] = unit<TOP>(q[0]);
        o[plane] = unit<TOP>(q[1]);
        o[2 * plane] = unit<TOP>(q[2]);
    }
    if (TOP == 255 && a.dst_u8 && wy >= 0 && wy < a.h && wx >= 0 && wx < a.w) {
        unsigned char* o = a.dst_u8 + ((long long)wy * a.w + wx) * 3;
        o[0] = (unsigned char)(a.bgr ? q[2] : q[0]);
        o[1] = (unsigned char)q[1];
        o[2] = (unsigned char)(a.bgr ? q[0] : q[2]);
    }
}

// The walk of the crop: output rows 2k and 2k + 1, columns x .. x + 3
template <class PX, bool ALIGNED, bool LEFT>
__device__ __forceinline__ void decode_rows(const DecArgs& a, int k, int x) {
    constexpr int TOP = PX::TOP;
    const int wx = x - a.pad_left;                      // window column of the group's first pixel; outside = padding
    if (ALIGNED && PX::SUB != 0) {      // 4:2:2 / 4:4:4: every luma row has its own chroma row
        const int gx = a.x0 + clampi(wx, 0, a.w - 4);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * k + r;
            if (y >= a.Hp) break;
            const int fy = a.y0 + clampi(y - a.pad_top, 0, a.h - 1);
            int u[4], v[4], px[4][3];
            if (PX::SUB == 2) {
                sample_quad<PX>(a.yuv, a.uoff + (long long)fy * a.cs + gx, u);
                sample_quad<PX>(a.yuv, a.voff + (long long)fy * a.cs + gx, v);
            } else {
                load_row<PX>(a, fy, gx >> 1, u, v);
            }
            decode4<PX, LEFT>(a, fy, gx, u, u, v, v, px);
            store_group<TOP>(a, y, x, y - a.pad_top, wx, px);
        }
    } else if (ALIGNED) {
        const int gx = a.x0 + clampi(wx, 0, a.w - 4), q = gx >> 1;
        const int yA = 2 * k, yB = yA + 1;
        const int fyA = a.y0 + clampi(yA - a.pad_top, 0, a.h - 1), fyB = a.y0 + clampi(yB - a.pad_top, 0, a.h - 1);
        const int rA0 = fyA >> 1, rA1 = clampi(rA0 + ((fyA & 1) ? 1 : -1), 0, a.ch - 1);
        int uA0[4], uA1[4], vA0[4], vA1[4], px[4][3];
        load_row<PX>(a, rA0, q, uA0, vA0);
        load_row<PX>(a, rA1, q, uA1, vA1);
        decode4<PX, LEFT>(a, fyA, gx, uA0, uA1, vA0, vA1, px);
        store_group<TOP>(a, yA, x, yA - a.pad_top, wx, px);
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
                load_row<PX>(a, rB0, q, uB0, vB0);
            }
            if (rB1 == rA0 || rB1 == rA1) {
                const bool f = rB1 == rA0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uB1[i] = f ? uA0[i] : uA1[i];
                    vB1[i] = f ? vA0[i] : vA1[i];
                }
            } else {
                load_row<PX>(a, rB1, q, uB1, vB1);
            }
            decode4<PX, LEFT>(a, fyB, gx, uB0, uB1, vB0, vB1, px);
            store_group<TOP>(a, yB, x, yB - a.pad_top, wx, px);
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
                decode_pixel<PX, LEFT>(a, fy, a.x0 + clampi(wx + i, 0, a.w - 1), q);
                store_pixel<TOP>(a, y, x + i, wy, wx + i, q);
            }
        }
    }
}

template <class PX, bool ALIGNED, bool LEFT>
__global__ __launch_bounds__(256) void yuv420_crop_kernel(const DecArgs a) {
    const int total = a.rows * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int k = idx / a.groups;
        decode_rows<PX, ALIGNED, LEFT>(a, k, (idx - k * a.groups) * 4);
    }
}

// The arguments of mode 1, which reads packed frames only: DecArgs without the strides, which are the plane widths.  The kernel's
// argument block and with it its code are what they were before frames could have a pitch.  The window-and-sink half is DecOut itself;
// the frame half is converted by the two functions below the struct, and by nothing else.
struct AreaSrc {
    const unsigned char* yuv;
    int H, W, ch, cw;
    long long uoff, voff;
    int kY, kRV, kGU, kGV, kBU, yo, mid, T;
};
struct AreaArgs : AreaSrc, DecOut {};
inline AreaArgs area_args(const DecArgs& a) {
    return {{a.yuv, a.H, a.W, a.ch, a.cw, a.uoff, a.voff, a.kY, a.kRV, a.kGU, a.kGV, a.kBU, a.yo, a.mid, a.T}, a};
}
__device__ __forceinline__ DecArgs dec_args(const AreaArgs& p) {
    return {{p.yuv, p.H, p.W, p.ch, p.cw, p.uoff, p.voff, p.W, p.cw, 0, p.kY, p.kRV, p.kGU, p.kGV, p.kBU, p.yo, p.mid, p.T}, p};
}

// mode 1: four output pixels of one output row from source rows fy (even) and fy + 1, columns gx .. gx + 7
template <class PX, bool ALIGNED, bool LEFT>
__global__ __launch_bounds__(256) void yuv420_area_kernel(const AreaArgs p) {
    const DecArgs a = dec_args(p);
    const int total = a.rows * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        const int wy = y - a.pad_top, wx = x - a.pad_left;
        const int fy = a.y0 + 2 * clampi(wy, 0, a.h - 1);           // even: rows fy and fy + 1 share chroma row fy >> 1
        if (ALIGNED) {
            const int gx = a.x0 + 2 * clampi(wx, 0, a.w - 4);
            const int r = fy >> 1, rm = max(r - 1, 0), rp = min(r + 1, a.ch - 1);
            int px[4][3], u[3][6], v[3][6];         // the three chroma rows, six samples wide, loaded once for both halves
            load_seg<PX, true, 6>(a, a.uoff, rm, gx >> 1, u[0]);
            load_seg<PX, true, 6>(a, a.voff, rm, gx >> 1, v[0]);
            load_seg<PX, true, 6>(a, a.uoff, r, gx >> 1, u[1]);
            load_seg<PX, true, 6>(a, a.voff, r, gx >> 1, v[1]);
            load_seg<PX, true, 6>(a, a.uoff, rp, gx >> 1, u[2]);
            load_seg<PX, true, 6>(a, a.voff, rp, gx >> 1, v[2]);
#pragma unroll
            for (int half = 0; half < 2; ++half) {          // source columns gx + 4 half .. + 3 -> output pixels 2 half, 2 half + 1
                const int hx = gx + 4 * half, o = 2 * half;
                int top[4][3], bot[4][3];
                decode4<PX, LEFT>(a, fy, hx, u[1] + o, u[0] + o, v[1] + o, v[0] + o, top);            // even row: (r, r - 1), weights (3, 1)
                decode4<PX, LEFT>(a, fy + 1, hx, u[1] + o, u[2] + o, v[1] + o, v[2] + o, bot);        // odd row: (r, r + 1)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[2 * half + j][c] = (top[2 * j][c] + top[2 * j + 1][c] + bot[2 * j][c] + bot[2 * j + 1][c] + 2) >> 2;
            }
            store_group<255>(a, y, x, wy, wx, px);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.Wp) break;
                const int fx = a.x0 + 2 * clampi(wx + i, 0, a.w - 1);
                int s[4][3], q[3];
                decode_pixel<PX, LEFT>(a, fy, fx, s[0]);
                decode_pixel<PX, LEFT>(a, fy, fx + 1, s[1]);
                decode_pixel<PX, LEFT>(a, fy + 1, fx, s[2]);
                decode_pixel<PX, LEFT>(a, fy + 1, fx + 1, s[3]);
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c] = (s[0][c] + s[1][c] + s[2][c] + s[3][c] + 2) >> 2;
                store_pixel<255>(a, y, x + i, wy, wx + i, q);
            }
        }
    }
}

// Launches the decode of a checked window.  aligned path: Y groups are dwords, chroma pairs naturally aligned (cw even, group origins
// even), plane stores 16 bytes, RGB groups three dwords; a group of four lies wholly inside the window or wholly in the padding
// (without a canvas Wp is w and pad_left 0)
// The run-time properties select the instance in this one place; decode_instance (yuv_common.h) names the combinations that have none,
// and mode 1 exists for the planar LSB 4:2:0 pixels 0..255 alone.  atmvfi_yuv_decode has refused the rest.
void launch_decode(const DecArgs& a, const atmvfi_yuv_desc& d, bool keep, int mode, void* stream) {
    const bool al = aligned4(a.yuv) && a.W % 4 == 0 && layout_aligned(a.ys, a.cs, a.uoff, a.voff, d) && a.x0 % 4 == 0 && a.w % 4 == 0 &&
                    (!a.dst || canvas_aligned(a.dst, a.Wp, a.pad_left)) && (!a.dst_u8 || aligned4(a.dst_u8));
    const dim3 grid = yuv_grid((long long)a.rows * a.groups), block(256);
    const hipStream_t st = (hipStream_t)stream;
    dispatch_sub([&](auto SUBC, auto AL, auto LEFT, auto D10, auto KEEP, auto IL, auto MSB) {
        constexpr int DEPTH = D10() ? 10 : 8, TOP = KEEP() ? 1023 : 255, SUB = SUBC();
        if constexpr (decode_instance<DEPTH, TOP, IL(), MSB(), SUB, LEFT()>) {
            using PX = Pixel<DEPTH, TOP, IL(), MSB(), SUB>;
            if (mode == 0) {
                hipLaunchKernelGGL((yuv420_crop_kernel<PX, AL(), LEFT()>), grid, block, 0, st, a);
                return;
            }
            if constexpr (TOP == 255 && !IL() && !MSB() && SUB == 0)
                hipLaunchKernelGGL((yuv420_area_kernel<PX, AL(), LEFT()>), grid, block, 0, st, area_args(a));
        }
    }, d.subsampling, al, d.siting != 0, d.depth == 10, keep, d.chroma != 0, d.msb != 0);
}

}  // namespace

// The one host path of every decode: the checks in one order, the geometry, the launch.  The descriptor says what the frame is (all
// zero but H, W, depth, matrix: the packed planar 4:2:0 frame); mode 1 (area 2x: the window reads 2h x 2w source pixels, a lane makes
// one output row) reads packed planar LSB 4:2:0 frames to pixels 0..255.
extern "C" int atmvfi_yuv_decode(const atmvfi_yuv_desc* desc, const void* yuv, int keep_depth, int mode, int y0, int x0, int h, int w, void* dst_u8,
                                 int bgr, float* dst, int Hp, int Wp, int pad_top, int pad_left, void* stream) {
    const char* me = "yuv_decode";
    ATMVFI_REQUIRE(desc, ATMVFI_EINVAL, "%s: null descriptor", me);
    const atmvfi_yuv_desc& d = *desc;
    if (d.subsampling != 0)
        if (const int rc = check_sub(me, d)) return rc;
    ATMVFI_REQUIRE(yuv, ATMVFI_EINVAL, "%s: null source", me);
    ATMVFI_REQUIRE(dst || dst_u8, ATMVFI_EINVAL, "%s: both outputs are null (give dst, dst_u8 or both)", me);
    if (const int rc = check_format(me, d)) return rc;
    if (const int rc = check_depth(me, d)) return rc;
    Layout l;
    if (const int rc = check_surface(me, d, &l)) return rc;
    const int H = d.H, W = d.W, sub = d.subsampling;
    ATMVFI_REQUIRE(keep_depth == 0 || keep_depth == 1, ATMVFI_EINVAL, "%s: keep_depth must be 0 or 1 (got %d)", me, keep_depth);
    ATMVFI_REQUIRE(!(keep_depth && d.depth != 10), ATMVFI_EINVAL, "%s: keep_depth needs a 10-bit surface", me);
    ATMVFI_REQUIRE(!(keep_depth && dst_u8), ATMVFI_EINVAL, "%s: dst_u8 holds 8-bit pixels: not with keep_depth", me);
    ATMVFI_REQUIRE(mode == 0 || mode == 1, ATMVFI_EINVAL, "%s: unknown mode %d (0: crop, 1: area 2x)", me, mode);
    ATMVFI_REQUIRE(mode == 0 || (sub == 0 && d.chroma == 0 && !d.msb && !d.pitch && !d.chroma_pitch && !d.chroma_offset && !keep_depth), ATMVFI_EINVAL,
                   "%s: mode 1 reads packed planar 4:2:0 frames with LSB samples, to pixels 0..255", me);
    ATMVFI_REQUIRE(h >= 1 && w >= 1, ATMVFI_EINVAL, "%s: negative or zero size: the window's h and w must be at least 1 (got %d x %d)", me, h, w);
    // (the wording serves two contracts: callers match "negative or zero" for a negative origin, or "outside the")
    ATMVFI_REQUIRE(y0 >= 0 && x0 >= 0, ATMVFI_EINVAL,
                   "%s: the window's origin (%d, %d) is negative, outside the frame (refused like a negative or zero size)", me, y0, x0);
    const long long s = mode == 1 ? 2 : 1;
    ATMVFI_REQUIRE(y0 + s * h <= H && x0 + s * w <= W, ATMVFI_EINVAL,
                   "%s: window outside the frame (mode %d reads %lld x %lld source pixels at (%d, %d) of a %d x %d frame)", me, mode, s * h, s * w,
                   y0, x0, H, W);
    if (sub == 0) ATMVFI_REQUIRE(y0 % 2 == 0 && x0 % 2 == 0, ATMVFI_EINVAL, "%s: the window origin (%d, %d) must be even", me, y0, x0);
    if (sub == 1) ATMVFI_REQUIRE(x0 % 2 == 0, ATMVFI_EINVAL, "%s: the window origin (%d, %d) must have an even x0 for 4:2:2 frames", me, y0, x0);
    if (dst) {
        if (const int rc = check_canvas(me, "dst", "window", dst, h, w, Hp, Wp, pad_top, pad_left)) return rc;
    } else {        // no canvas: the output geometry is the window's
        Hp = h;
        Wp = w;
        pad_top = pad_left = 0;
    }
    const int groups = groups_of(Wp), rows = mode == 1 ? Hp : pairs_of(Hp);
    if (const int rc = check_items(me, rows, groups, "output of", Hp, Wp)) return rc;
    const DecArgs a = {make_src(yuv, d, keep_depth != 0, l), {y0, x0, h, w, dst, Hp, Wp, pad_top, pad_left, (unsigned char*)dst_u8, bgr ? 1 : 0, groups, rows}};
    launch_decode(a, d, keep_depth != 0, mode, stream);
    return atmvfi::check_launch(me);
}
