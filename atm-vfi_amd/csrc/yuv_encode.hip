// RGB -> YUV 4:2:0 (and planar 4:2:2 / 4:4:4): atmvfi_yuv_encode of include/atmvfi.h, one kernel family behind one checked host path
// (surface_encode, below the kernel).  yuv_common.h holds the definition and the shared helpers; yuv.hip is the other direction.  The
// frame descriptor (atmvfi_yuv_desc) selects what runs:
//   depth 8                   uint8 [H,W,3] (RGB or BGR) or the fp32 canvas in units of 1 / 255 -> 8-bit samples
//   depth 10                  the fp32 canvas in units of 1 / 1023 -> 10-bit samples, the depth kept
//   chroma / msb              either of the two into a tight surface: planar, or NV12 / NV21 / P010 (interleaved chroma, msb samples);
//                             a lane's two chroma samples of both planes leave as ONE dword (8 bit) or 8-byte (10 bit) store
//   subsampling 1 / 2         planar 4:2:2 / 4:4:4 frames (SUB = 1 / 2).  The lane's 4 x 2 block makes
//                             a chroma pair per plane and ROW (4:2:2: a 2-byte or dword store) or a chroma group per plane and row
//                             (4:4:4: a dword or 8-byte store, as the Y group)
//
// Bandwidth-bound: from fp32 12 B/px in and 1.5 or 3 out.  A lane owns a 4 x 2 luma block of the frame: two Y groups and two chroma
// samples per plane; left siting reads one more pixel column.
//   aligned path (frame pointer 4-byte aligned, W % 4 == 0; the uint8 source 4-byte aligned, or the fp32 canvas 16-byte aligned with
//           Wp % 4 == 0 and pad_left % 4 == 0): the source group is three dwords or three 16-byte loads, a Y group one dword or 8-byte
//           store, a chroma pair (cw even) one 2-byte or dword store;
//   general path: any geometry and alignment: byte accesses to the frame, scalar loads, the same integer arithmetic, the same bits.
// Vector stores only, no atomics, nothing pre-zeroed: every output byte is written by exactly one lane.
#include "yuv_common.h"

namespace {

enum Source { SRC_U8, SRC_F255, SRC_F1023 };       // the pixel: uint8, clip(rint(x * 255)), clip(rint(x * 1023))

struct EncArgs {
    const unsigned char* src_u8;
    int bgr;
    const float* src;
    int Hp, Wp, pad_top, pad_left;
    int H, W, ch, cw;
    int eY[3], eU[3], eV[3], yo;
    unsigned char* yuv;
    long long uoff, voff;       // first U / V sample, in samples (interleaved chroma: one is the other plus 1)
    int ys, cs;                 // row strides of the luma and the chroma plane(s), in samples
    int vu;                     // interleaved chroma, V first
    int groups;                 // ceil(W / 4); a group makes chroma columns 2g and 2g + 1
};

template <int SRC>
__device__ __forceinline__ void load_px(const EncArgs& a, int fy, int fx, int p[3]) {
    if (SRC == SRC_U8) {
        const unsigned char* s = a.src_u8 + ((long long)fy * a.W + fx) * 3;
        p[0] = a.bgr ? s[2] : s[0];
        p[1] = s[1];
        p[2] = a.bgr ? s[0] : s[2];
    } else {        // rint: half to even, as np.rint (frame_f32_to_u8); the conversion saturates
        constexpr int TOP = SRC == SRC_F1023 ? 1023 : 255;
        const long long plane = (long long)a.Hp * a.Wp;
        const float* s = a.src + (long long)(fy + a.pad_top) * a.Wp + (fx + a.pad_left);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = clampi(__float2int_rn(s[c * plane] * (float)TOP), 0, TOP);
    }
}

template <int SRC>
__device__ __forceinline__ void load_px4_aligned(const EncArgs& a, int fy, int fx, int p[4][3]) {
    if (SRC == SRC_U8) {
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
    } else {
        constexpr int TOP = SRC == SRC_F1023 ? 1023 : 255;
        const long long plane = (long long)a.Hp * a.Wp;
        const float* s = a.src + (long long)(fy + a.pad_top) * a.Wp + (fx + a.pad_left);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(s + c * plane);
            const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) p[i][c] = clampi(__float2int_rn(f[i] * (float)TOP), 0, TOP);
        }
    }
}

// (__mul24: the full-rate 24-bit multiply; coefficients are below 2^17, samples and pixel sums below 2^14)
__device__ __forceinline__ int dot3(const int e[3], const int p[3]) { return __mul24(e[0], p[0]) + __mul24(e[1], p[1]) + __mul24(e[2], p[2]); }

// N samples of one plane row from sample i on: one aligned store of N samples (N = 2: a chroma pair; N = 4: a Y group), or its first n
// samples byte by byte
template <int DEPTH, bool ALIGNED, int N>
__device__ __forceinline__ void store_samples(unsigned char* yuv, long long i, const int v[N], int n) {
    if (ALIGNED) {
        if (DEPTH == 8) {
            unsigned d = 0u;
#pragma unroll
            for (int k = 0; k < N; ++k) d |= (unsigned)v[k] << (8 * k);
            if (N == 2) reinterpret_cast<U16x1*>(yuv + i)->v = (unsigned short)d;
            else *reinterpret_cast<unsigned*>(yuv + i) = d;
        } else {
            const unsigned d0 = (unsigned)v[0] | ((unsigned)v[1] << 16);
            if (N == 2) *reinterpret_cast<unsigned*>(yuv + 2 * i) = d0;
            else *reinterpret_cast<U32x2*>(yuv + 2 * i) = U32x2{d0, (unsigned)v[N - 2] | ((unsigned)v[N - 1] << 16)};
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (k >= n) break;
            if (DEPTH == 8) {
                yuv[i + k] = (unsigned char)v[k];
            } else {
                yuv[2 * (i + k)] = (unsigned char)(v[k] & 0xff);
                yuv[2 * (i + k) + 1] = (unsigned char)(v[k] >> 8);
            }
        }
    }
}

// IL: chroma is one plane of interleaved pairs; MSB: a 10-bit sample is stored as value << 6 (the low bits zero).  The planar, LSB
// instances compile to what they were without either.  SUB: 0 4:2:0, 1 4:2:2, 2 4:4:4 (planar, LSB): a.ch is H then, and the lane
// still owns luma rows 2j and 2j + 1.
template <int SRC, bool ALIGNED, bool LEFT, bool IL = false, bool MSB = false, int SUB = 0>
__global__ __launch_bounds__(256) void yuv420_encode_kernel(const EncArgs a) {
    constexpr int DEPTH = SRC == SRC_F1023 ? 10 : 8, TOP = SRC == SRC_F1023 ? 1023 : 255, MID = (TOP + 1) / 2, SH = MSB ? 6 : 0;
    static_assert(!MSB || DEPTH == 10, "only 10-bit samples are stored in the upper bits");
    static_assert(SUB == 0 || (SUB <= 2 && !IL && !MSB && !(SUB == 2 && LEFT)), "4:2:2 and 4:4:4 frames are planar with LSB samples");
    const int total = (SUB == 0 ? a.ch : (a.H + 1) >> 1) * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int j = idx / a.groups, g = idx - j * a.groups, x = 4 * g;
        int px[2][5][3];        // [row][0: the column left of the group (left siting only), 1..4: the group][R, G, B]
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int fy = min(2 * j + r, a.H - 1);
            if (LEFT) load_px<SRC>(a, fy, max(x - 1, 0), px[r][0]);
            else px[r][0][0] = px[r][0][1] = px[r][0][2] = 0;
            if (ALIGNED) {
                load_px4_aligned<SRC>(a, fy, x, &px[r][1]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) load_px<SRC>(a, fy, min(x + i, a.W - 1), px[r][1 + i]);
            }
        }
        // luma
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * j + r;
            if (y >= a.H) break;
            int Y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) Y[i] = clampi(((dot3(a.eY, px[r][1 + i]) + (1 << 13)) >> 14) + a.yo, 0, TOP) << SH;
            store_samples<DEPTH, ALIGNED, 4>(a.yuv, (long long)y * a.ys + x, Y, a.W - x);
        }
        if constexpr (SUB == 2) {       // 4:4:4: a chroma sample per pixel, from the pixel itself (sh = 0)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = 2 * j + r;
                if (y >= a.H) break;
                int U[4], V[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    U[i] = clampi(((dot3(a.eU, px[r][1 + i]) + (1 << 13)) >> 14) + MID, 0, TOP);
                    V[i] = clampi(((dot3(a.eV, px[r][1 + i]) + (1 << 13)) >> 14) + MID, 0, TOP);
                }
                const long long c0 = (long long)y * a.cs + x;
                store_samples<DEPTH, ALIGNED, 4>(a.yuv, a.uoff + c0, U, a.W - x);
                store_samples<DEPTH, ALIGNED, 4>(a.yuv, a.voff + c0, V, a.W - x);
            }
            continue;
        } else if constexpr (SUB == 1) {        // 4:2:2: chroma columns 2g and 2g + 1 of BOTH rows, the horizontal taps alone
            constexpr int sh1 = LEFT ? 2 : 1;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = 2 * j + r;
                if (y >= a.H) break;
                int U[2], V[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    int s[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        s[c] = LEFT ? px[r][2 * i][c] + 2 * px[r][1 + 2 * i][c] + px[r][2 + 2 * i][c] : px[r][1 + 2 * i][c] + px[r][2 + 2 * i][c];
                    U[i] = clampi(((dot3(a.eU, s) + (1 << (13 + sh1))) >> (14 + sh1)) + MID, 0, TOP);
                    V[i] = clampi(((dot3(a.eV, s) + (1 << (13 + sh1))) >> (14 + sh1)) + MID, 0, TOP);
                }
                const long long c0 = (long long)y * a.cs + 2 * g;      // (aligned: cw is even, both columns exist)
                store_samples<DEPTH, ALIGNED, 2>(a.yuv, a.uoff + c0, U, a.cw - 2 * g);
                store_samples<DEPTH, ALIGNED, 2>(a.yuv, a.voff + c0, V, a.cw - 2 * g);
            }
            continue;
        }
        // chroma columns 2g and 2g + 1
        constexpr int sh = LEFT ? 3 : 2;
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
            U[i] = clampi(((dot3(a.eU, s) + (1 << (13 + sh))) >> (14 + sh)) + MID, 0, TOP) << SH;
            V[i] = clampi(((dot3(a.eV, s) + (1 << (13 + sh))) >> (14 + sh)) + MID, 0, TOP) << SH;
        }
        if (IL) {       // both planes' two samples as one store of four: a dword, or 8 bytes at depth 10
            const int quad[4] = {a.vu ? V[0] : U[0], a.vu ? U[0] : V[0], a.vu ? V[1] : U[1], a.vu ? U[1] : V[1]};
            store_samples<DEPTH, ALIGNED, 4>(a.yuv, a.uoff - a.vu + (long long)j * a.cs + 4 * g, quad, 2 * (a.cw - 2 * g));
        } else {
            const long long c0 = (long long)j * a.cs + 2 * g;      // (aligned: cw is even, both columns exist)
            store_samples<DEPTH, ALIGNED, 2>(a.yuv, a.uoff + c0, U, a.cw - 2 * g);
            store_samples<DEPTH, ALIGNED, 2>(a.yuv, a.voff + c0, V, a.cw - 2 * g);
        }
    }
}

// the encode instances that exist (launch_encode walks the whole family and compiles these): as decode_instance
template <int SRC, bool IL, bool MSB, int SUB, bool LEFT>
constexpr bool encode_instance = (!MSB || SRC == SRC_F1023) && (SUB == 0 || (!IL && !MSB)) && !(SUB == 2 && LEFT);

// Where an encode writes: the TIGHT frame at `yuv` -- the picture's own (FH x FW = H x W, origin 0) or, for atmvfi_yuv_compose, a larger
// frame in which the picture is the window at (y0, x0): the kernel gets the window's first luma sample as its base and the chroma
// origins relative to it, with the FRAME's row strides.  Nothing else of the kernel knows about the frame.
struct Place {
    int FH, FW, y0, x0;
};

// Launches the encode of a checked frame `d`; exactly one of src_u8 and src is given.  The destination is tight: chroma 0 is the packed
// planar frame, 1 / 2 the interleaved surface (U / V first); msb: 10-bit samples stored in the upper bits; subsampling 1 4:2:2, 2 4:4:4.
// The run-time properties select the instance in this one place: the source is fp32 x 1023 at depth 10, else fp32 x 255 or uint8;
// msb samples come from the 10-bit source alone, 4:2:2 / 4:4:4 are planar LSB, and 4:4:4 has no siting.
void launch_encode(const atmvfi_yuv_desc& d, const void* src_u8, int bgr, const float* src, int Hp, int Wp, int pad_top, int pad_left, void* yuv,
                   void* stream, const Place& at) {
    const int H = d.H, W = d.W, depth = d.depth, chroma = d.chroma, sub = d.subsampling;
    const Coeffs& c = depth == 10 ? kCoeffs10[d.matrix] : kCoeffs[d.matrix][d.full_range];
    const int ch = chroma_rows(H, sub), cw = chroma_cols(W, sub), groups = groups_of(W), b = depth == 10 ? 2 : 1;
    EncArgs a = {(const unsigned char*)src_u8, src_u8 && bgr ? 1 : 0, src, Hp, Wp, pad_top, pad_left, H, W, ch, cw};
    for (int k = 0; k < 3; ++k) {
        a.eY[k] = c.enc[0][k];
        a.eU[k] = c.enc[1][k];
        a.eV[k] = c.enc[2][k];
    }
    a.yo = depth == 10 ? 64 : (d.full_range ? 0 : 16);
    const Layout l = tight_layout(at.FH, at.FW, chroma, sub);
    // the window's origin in samples: of the luma plane, and of a chroma plane (an interleaved column is two samples)
    const long long yorg = (long long)at.y0 * l.ys + at.x0;
    const long long corg = (long long)(sub == 0 ? at.y0 / 2 : at.y0) * l.cs + (sub == 2 ? at.x0 : at.x0 / 2) * (chroma ? 2 : 1);
    const long long uabs = l.uoff + corg + (chroma == 2 ? 1 : 0);
    const long long vabs = chroma == 0 ? l.uoff + corg + (long long)chroma_rows(at.FH, sub) * l.cs : l.uoff + corg + (chroma == 1 ? 1 : 0);
    a.yuv = (unsigned char*)yuv + yorg * b;
    a.uoff = uabs - yorg;
    a.voff = vabs - yorg;
    a.ys = l.ys;
    a.cs = l.cs;
    a.vu = chroma == 2 ? 1 : 0;
    a.groups = groups;
    // (a tight frame of its own with W % 4 == 0: the layout follows from the pointer; a window must also start on a group)
    const bool al = aligned4(yuv) && W % 4 == 0 && (yorg * b) % 4 == 0 && layout_aligned(l.ys, l.cs, uabs, vabs, d) &&
                    (src ? canvas_aligned(src, Wp, pad_left) : aligned4(src_u8));
    const dim3 grid = yuv_grid((long long)pairs_of(H) * groups), block(256);
    dispatch_sub([&](auto SUB, auto AL, auto LEFT, auto D10, auto F32, auto IL, auto MSB) {
        constexpr int SRC = D10() ? SRC_F1023 : (F32() ? SRC_F255 : SRC_U8);
        if constexpr ((F32() || !D10()) && encode_instance<SRC, IL(), MSB(), SUB(), LEFT()>)
            hipLaunchKernelGGL((yuv420_encode_kernel<SRC, AL(), LEFT(), IL(), MSB(), SUB()>), grid, block, 0, (hipStream_t)stream, a);
    }, sub, al, d.siting != 0, depth == 10, src != nullptr, chroma != 0, d.msb != 0);
}

// The one host path of every encode, under the caller's name `me`: the checks in one order, then the launch.  `d` describes the tight
// destination (its strides are not read); `window`: the frame `d` is a window of (atmvfi::yuv_encode_window).
int surface_encode(const char* me, const atmvfi_yuv_desc& d, const void* src_u8, int bgr, const float* src, int Hp, int Wp, int pad_top,
                   int pad_left, void* yuv, void* stream, const Place* window = nullptr) {
    if (d.subsampling != 0)
        if (const int rc = check_sub(me, d)) return rc;
    ATMVFI_REQUIRE(yuv, ATMVFI_EINVAL, "%s: null destination", me);
    ATMVFI_REQUIRE((src_u8 != nullptr) != (src != nullptr), ATMVFI_EINVAL, "%s: give exactly one of src_u8 and src (got %s)", me,
                   src_u8 ? "both" : "neither");
    if (const int rc = check_format(me, d)) return rc;
    if (const int rc = check_depth(me, d)) return rc;
    Layout l;
    if (const int rc = check_surface(me, d, &l, true)) return rc;
    ATMVFI_REQUIRE(!(d.depth == 10 && src_u8), ATMVFI_EINVAL, "%s: a 10-bit surface is encoded from the fp32 canvas (src), not from src_u8", me);
    if (src)
        if (const int rc = check_canvas(me, "src", "frame", src, d.H, d.W, Hp, Wp, pad_top, pad_left)) return rc;
    if (const int rc = check_items(me, (d.H + 1) / 2, groups_of(d.W), "a frame of", d.H, d.W)) return rc;
    launch_encode(d, src_u8, bgr, src, Hp, Wp, pad_top, pad_left, yuv, stream, window ? *window : Place{d.H, d.W, 0, 0});
    return atmvfi::check_launch(me);
}

}  // namespace

extern "C" int atmvfi_yuv_encode(const atmvfi_yuv_desc* desc, const void* src_u8, int bgr, const float* src, int Hp, int Wp, int pad_top,
                                 int pad_left, void* yuv, void* stream) {
    ATMVFI_REQUIRE(desc, ATMVFI_EINVAL, "yuv_encode: null descriptor");
    return surface_encode("yuv_encode", *desc, src_u8, bgr, src, Hp, Wp, pad_top, pad_left, yuv, stream);
}

// atmvfi_yuv_compose's window (active.hip has checked that it lies in the frame `d`, on the subsampling's grid): the h x w picture as a
// frame of the cropped format -- the checks and the kernel of atmvfi_yuv_encode -- written at (y0, x0) of the tight frame of `d`
int atmvfi::yuv_encode_window(const char* me, const atmvfi_yuv_desc& d, void* frame, int y0, int x0, int h, int w, const void* src_u8,
                              const float* src, int Hp, int Wp, int pad_top, int pad_left, void* stream) {
    atmvfi_yuv_desc win = d;
    win.H = h;
    win.W = w;
    const Place at = {d.H, d.W, y0, x0};
    return surface_encode(me, win, src_u8, 0, src, Hp, Wp, pad_top, pad_left, frame, stream, &at);
}
