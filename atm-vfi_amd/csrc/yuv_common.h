// YUV 4:2:0 (planar I420, and the decoder surfaces NV12 / NV21 / P010) <-> RGB at the host boundary of the video loops and of the Y4M
// evaluations: the definition, its device helpers and the host-side checks, shared by yuv.hip (atmvfi_yuv_decode) and yuv_encode.hip
// (atmvfi_yuv_encode); include/atmvfi.h declares them and the frame descriptor (atmvfi_yuv_desc) that every host function here takes;
// atm-vfi_amd/yuv.py holds the numpy twins.  Nothing of the reference: its scripts take PNGs.  The definition is the project's own, in int32 throughout (>> floors), so the
// device, the vectorised numpy twins and the per-pixel models (tests/cpu_yuv.py, cpu_yuv10.py, cpu_yuv_window.py) agree bit for bit;
// every kernel runs the functions below, so two entry points that decode the same pixel give the same bits by construction.
//   frame     Y [H,W], U [ch,cw], V [ch,cw] back to back, ch = (H + 1) / 2, cw = (W + 1) / 2; uint8, or little-endian uint16 (0..1023)
//             for depth 10
//   pixel     8 bit (Pixel<8, 255>): RGB 0..255 (top = 255), yo = 16 (limited) or 0 (full range), mid = 128, T = 14; fp32 is q / 255
//             10 -> 8 bit (Pixel<10, 255>): 10-bit limited-range samples to RGB 0..255 (decode only): yo = 64, mid = 512, T = 16, the 8-bit matrix
//             10 bit kept (Pixel<10, 1023>): RGB 0..1023 (top = 1023), yo = 64, mid = 512, T = 14, the matrix of kCoeffs10; fp32 is q / 1023
//   decode    chroma of luma pixel (y, x): rows r0 = y >> 1 and r1 = clamp(r0 + (y & 1 ? 1 : -1)) with weights (3, 1); columns
//             centre-sited q0 = x >> 1, q1 = clamp(q0 + (x & 1 ? 1 : -1)), weights (3, 1); left-sited q0, q1 = min(q0 + 1, cw - 1),
//             weights (4, 0) for even and (2, 2) for odd x; c' = (wy0 (wx0 c00 + wx1 c01) + wy1 (wx0 c10 + wx1 c11) + 8) >> 4;
//             R = clip((kY y + kRV v + 2^(T-1)) >> T), G = clip((kY y + kGU u + kGV v + ..) >> T), B = clip((kY y + kBU u + ..) >> T)
//             with y = Y - yo, u = U' - mid, v = V' - mid and clip to 0..top; the fp32 output is q / top with the bits of the fp32
//             division.  A decode takes the window (y0, x0, h, w) of the frame (even origin) to (pad_top, pad_left) of the canvas,
//             replicate padding by clamping the output coordinate INTO THE WINDOW; chroma neighbours clamp at the FRAME's edges: the
//             window is a window of the whole frame's decode.
//   encode    source pixel p: the uint8 RGB value, or from fp32 clip(rint(fl32(x * top))), half to even (frame_f32_to_u8's pixel);
//             Y = clip(((eY . p + 2^13) >> 14) + yo); chroma sample (j, i) from the un-rounded sums s over rows 2j, min(2j + 1, H - 1) and
//             columns 2i, min(2i + 1, W - 1) (centre, sh = 2) or max(2i - 1, 0), 2i, min(2i + 1, W - 1) weighted 1, 2, 1 (left, sh = 3):
//             U = clip(((eU . s + 2^(13 + sh)) >> (14 + sh)) + mid), V alike
//   surface   where the samples of a frame lie (the descriptor's chroma, msb and three strides; yuv.py: Surface; model
//             tests/cpu_yuv_surface.py): chroma as two planes or as ONE plane of interleaved pairs, U first (NV12, P010) or V first
//             (NV21); 10-bit samples in the low or, msb, in the upper ten bits of their word (read s >> 6, written v << 6); rows at a
//             pitch, chroma from an offset.  YuvSrc carries the strides and the U / V origins (V first is U first with the origins
//             swapped); interleaved and msb are properties of the instance (Pixel), as the siting is.  The arithmetic above is applied
//             to the samples found there, unchanged.  A decoder's surface that already lies in device memory is decoded in place: its
//             pointer, pitch and chroma offset go to atmvfi_yuv_decode, no padding byte is read and nothing is repacked.
//   4:2:2 / 4:4:4   (the descriptor's subsampling; yuv.py: Format.subsampling; model tests/cpu_yuv_sub.py) planar frames
//             whose chroma planes are [H, cw] (4:2:2) or [H, W] (4:4:4): SUB, one more property of the instance.  Decode 4:2:2: row y, the
//             columns and weights above, c' = (wx0 c[y][q0] + wx1 c[y][q1] + 2) >> 2; 4:4:4: c' = c[y][x].  Encode: the horizontal
//             taps above over ONE row (4:2:2: sh = 1 centre, 2 left) or the pixel itself (4:4:4: sh = 0).  The same coefficients,
//             offsets and clips; a 4:2:2 frame of equal chroma rows decodes as the 4:2:0 frame of those rows ((4 h + 8) >> 4 is
//             (h + 2) >> 2), and a picture of equal row pairs encodes to the 4:2:0 chroma ((2 s + 2^(k+1)) >> (k+1) is (s + 2^k) >> k).
// Library-wide rules, here as everywhere: vector stores only, no atomics, nothing pre-zeroed: every output byte is written by exactly
// one lane.
#pragma once
#include <type_traits>

#include "common.h"

namespace atmvfi {
// yuv_encode.hip, for active.hip (atmvfi_yuv_compose): the encode kernel with a destination origin inside the larger tight frame of `d`
int yuv_encode_window(const char* me, const atmvfi_yuv_desc& d, void* frame, int y0, int x0, int h, int w, const void* src_u8, const float* src,
                      int Hp, int Wp, int pad_top, int pad_left, void* stream);
}  // namespace atmvfi

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
// the same with the depth kept: luma scaled by 876 / 1023 and chroma by 896 / 1023 (yuv.py: COEFFS10; tests/test_yuv10_cpu.py holds
// both to the table of the README and the header)
const Coeffs kCoeffs10[2] = {     // [matrix]
    {{19133, 26226, -6438, -13359, 33148}, {{4195, 8235, 1599}, {-2421, -4754, 7175}, {7175, -6008, -1167}}},
    {{19133, 29459, -3504, -8757, 34711}, {{2983, 10034, 1013}, {-1644, -5531, 7175}, {7175, -6517, -658}}},
};

// ------------------------------------------------------------------------------------------------------------------ device: decode
// the resident frame and the constants of its pixel: the first members of every decode kernel's arguments
struct YuvSrc {
    const unsigned char* yuv;
    int H, W, ch, cw;
    long long uoff, voff;       // first U / V sample, in samples (interleaved chroma: one is the other plus 1)
    int ys, cs;                 // row strides of the luma and the chroma plane(s), in samples
    int vu;                     // interleaved chroma, V first (voff + 1 == uoff): the aligned path loads pairs and swaps afterwards
    int kY, kRV, kGU, kGV, kBU, yo, mid, T;
};
// the pixel kind of a decode instance: the frame's sample depth, the RGB pixel's maximum and how the samples lie in memory.  A template
// parameter, not a member of YuvSrc: with a constant maximum the clip is one v_med3_i32, and the decodes are bound by their
// instruction count.  IL: chroma is one plane of interleaved pairs (NV12 / NV21 / P010) instead of two planes; MSB: a 10-bit sample is
// stored as value << 6 (P010) and read as s >> 6.  The planar, LSB instances compile to what they were without either.  SUB: the
// chroma subsampling, 0 4:2:0, 1 4:2:2, 2 4:4:4 (planar, LSB only); the 4:2:0 instances compile to what they were without it.
template <int DEPTH_, int TOP_, bool IL_ = false, bool MSB_ = false, int SUB_ = 0>
struct Pixel {
    static constexpr int DEPTH = DEPTH_, TOP = TOP_, SUB = SUB_;
    static constexpr bool IL = IL_, MSB = MSB_;
    static_assert(SUB == 0 || (SUB <= 2 && !IL && !MSB), "4:2:2 and 4:4:4 frames are planar with LSB samples");
    static_assert((DEPTH == 8 || DEPTH == 10) && (TOP == 255 || (TOP == 1023 && DEPTH == 10)), "8 bit, 10 -> 8 bit or 10 bit kept");
    static_assert(!MSB || DEPTH == 10, "only 10-bit samples are stored in the upper bits");
};
// the decode instances that exist (launch_decode walks the whole family and compiles these): Pixel's own conditions, and 4:4:4 has no siting
template <int DEPTH, int TOP, bool IL, bool MSB, int SUB, bool LEFT>
constexpr bool decode_instance = (TOP == 255 || DEPTH == 10) && (!MSB || DEPTH == 10) && (SUB == 0 || (!IL && !MSB)) && !(SUB == 2 && LEFT);

// the layout of a surface, on the host: chroma 0 planar, 1 interleaved U first, 2 interleaved V first; strides in samples, uoff the
// first chroma row's first sample.  A packed I420 frame is tight_layout(H, W, 0).
struct Layout {
    int chroma;
    int ys, cs;
    long long uoff;
};
inline int chroma_rows(int H, int sub) { return sub == 0 ? (H + 1) / 2 : H; }
inline int chroma_cols(int W, int sub) { return sub == 2 ? W : (W + 1) / 2; }
inline Layout tight_layout(int H, int W, int chroma, int sub = 0) {
    const int cw = chroma_cols(W, sub);
    return Layout{chroma, W, chroma ? 2 * cw : cw, (long long)H * W};
}

// keep: the 10-bit depth kept (RGB 0..1023); otherwise RGB 0..255 from samples of either depth
inline YuvSrc make_src(const void* yuv, const atmvfi_yuv_desc& d, bool keep, const Layout& l) {
    const int H = d.H, W = d.W, depth = d.depth, full_range = d.full_range;
    const int ch = chroma_rows(H, d.subsampling), cw = chroma_cols(W, d.subsampling);
    const Coeffs& c = keep ? kCoeffs10[d.matrix] : kCoeffs[d.matrix][full_range];
    const long long uoff = l.uoff + (l.chroma == 2 ? 1 : 0), voff = l.chroma == 0 ? l.uoff + (long long)ch * l.cs : l.uoff + (l.chroma == 1 ? 1 : 0);
    return YuvSrc{(const unsigned char*)yuv, H, W, ch, cw, uoff, voff, l.ys, l.cs, l.chroma == 2 ? 1 : 0,
                  c.dec[0], c.dec[1], c.dec[2], c.dec[3], c.dec[4], depth == 10 ? 64 : (full_range ? 0 : 16), depth == 10 ? 512 : 128,
                  depth == 10 && !keep ? 16 : 14};
}

// the value of a stored 16-bit sample: its upper ten bits for MSB
template <bool MSB>
__device__ __forceinline__ int lo16(unsigned v) { return (int)((v & 0xffffu) >> (MSB ? 6 : 0)); }
template <bool MSB>
__device__ __forceinline__ int hi16(unsigned v) { return (int)(v >> (MSB ? 22 : 16)); }

template <class PX, bool AL>
__device__ __forceinline__ int sample(const unsigned char* p, long long i) {
    if (PX::DEPTH == 8) return p[i];
    if (AL) return lo16<PX::MSB>(reinterpret_cast<const unsigned short*>(p)[i]);
    return lo16<PX::MSB>((unsigned)p[2 * i] | ((unsigned)p[2 * i + 1] << 8));
}

// the naturally aligned pair of samples (i, i + 1) of the aligned paths: two bytes or one dword
template <class PX>
__device__ __forceinline__ void sample_pair(const unsigned char* p, long long i, int& s0, int& s1) {
    if (PX::DEPTH == 8) {
        const unsigned v = reinterpret_cast<const U16x1*>(p + i)->v;
        s0 = (int)(v & 0xffu);
        s1 = (int)(v >> 8);
    } else {
        const unsigned v = *reinterpret_cast<const unsigned*>(p + 2 * i);
        s0 = lo16<PX::MSB>(v);
        s1 = hi16<PX::MSB>(v);
    }
}

// the naturally aligned group of samples (i .. i + 3) of the aligned paths: one dword or one 8-byte load
template <class PX>
__device__ __forceinline__ void sample_quad(const unsigned char* p, long long i, int s[4]) {
    if (PX::DEPTH == 8) {
        const unsigned d = *reinterpret_cast<const unsigned*>(p + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = (int)((d >> (8 * k)) & 0xffu);
    } else {
        const U32x2 d = *reinterpret_cast<const U32x2*>(p + 2 * i);
        s[0] = lo16<PX::MSB>(d.a);
        s[1] = hi16<PX::MSB>(d.a);
        s[2] = lo16<PX::MSB>(d.b);
        s[3] = hi16<PX::MSB>(d.b);
    }
}

// seg[k] = plane[r][clamp(q - 1 + k, 0, cw - 1)], k = 0 .. N - 1: every chroma column that luma columns 2q .. 2q + 2N - 5 touch
// (N = 4: one group of four pixels; N = 6: two groups, seg + 2 being the second group's segment); planar chroma
template <class PX, bool AL, int N = 4>
__device__ __forceinline__ void load_seg(const YuvSrc& a, long long plane, int r, int q, int seg[N]) {
    const long long row = plane + (long long)r * a.cs;
    if (AL) {       // q even, the row's origin even: the columns q .. q + N - 3 are naturally aligned pairs inside the row
        seg[0] = sample<PX, true>(a.yuv, row + max(q - 1, 0));
#pragma unroll
        for (int p = 0; p < N - 2; p += 2) sample_pair<PX>(a.yuv, row + q + p, seg[1 + p], seg[2 + p]);
        seg[N - 1] = sample<PX, true>(a.yuv, row + min(q + N - 2, a.cw - 1));
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) seg[k] = sample<PX, false>(a.yuv, row + clampi(q - 1 + k, 0, a.cw - 1));
    }
}

// the same four columns of chroma row r for BOTH planes on the aligned paths.  Interleaved chroma: the row is loaded once -- the
// aligned centre pairs (first, second)[q], (first, second)[q + 1] as one dword (8 bit) or one 8-byte load (10 bit), each outer column
// as one 2-byte or dword load: three loads where two planes take six.  first / second are U / V, or V / U when a.vu: decode4 swaps.
template <class PX>
__device__ __forceinline__ void load_row(const YuvSrc& a, int r, int q, int u[4], int v[4]) {
    if (!PX::IL) {
        load_seg<PX, true>(a, a.uoff, r, q, u);
        load_seg<PX, true>(a, a.voff, r, q, v);
    } else {
        const long long row = a.uoff - a.vu + (long long)r * a.cs;
        sample_pair<PX>(a.yuv, row + 2 * max(q - 1, 0), u[0], v[0]);
        if (PX::DEPTH == 8) {
            const unsigned d = *reinterpret_cast<const unsigned*>(a.yuv + row + 2 * q);
            u[1] = (int)(d & 0xffu);
            v[1] = (int)((d >> 8) & 0xffu);
            u[2] = (int)((d >> 16) & 0xffu);
            v[2] = (int)(d >> 24);
        } else {
            const U32x2 d = *reinterpret_cast<const U32x2*>(a.yuv + 2 * (row + 2 * q));
            u[1] = lo16<PX::MSB>(d.a);
            v[1] = hi16<PX::MSB>(d.a);
            u[2] = lo16<PX::MSB>(d.b);
            v[2] = hi16<PX::MSB>(d.b);
        }
        sample_pair<PX>(a.yuv, row + 2 * min(q + 2, a.cw - 1), u[3], v[3]);
    }
}

// q / 255 for an integer q in 0..255 with the bits of the fp32 division (what frame_u8_to_f32 computes): q * r with r = fl(1 / 255), then
// one correction step in fused multiply-adds -- e = fl(q - 255 y), y + e r.  Equal to the division for all 256 values
// (tests/test_yuv_cpu.py checks every one in exact rational arithmetic); four instructions where the division's expansion takes ten, and
// the decode is bound by its instruction count, not by HBM, while it divides (tools/bench_yuv.py).
__device__ __forceinline__ float q255(int q) {
    const float f = (float)q, r = 0x1.010102p-8f;
    const float y = f * r;
    return __fmaf_rn(__fmaf_rn(-255.0f, y, f), r, y);
}
// q / 1023 for q in 0..1023, the same way with r = fl(1 / 1023): equal to the division for all 1024 values (tests/test_yuv10_cpu.py)
__device__ __forceinline__ float q1023(int q) {
    const float f = (float)q, r = 0x1.00401p-10f;
    const float y = f * r;
    return __fmaf_rn(__fmaf_rn(-1023.0f, y, f), r, y);
}
// the pixel's maximum as a template parameter: the fp32 value of an integer pixel
template <int TOP>
__device__ __forceinline__ float unit(int q) {
    return TOP == 255 ? q255(q) : q1023(q);
}

__device__ __forceinline__ int chroma_mix(int c00, int c01, int c10, int c11, int wx0, int wx1) {
    return (3 * (wx0 * c00 + wx1 * c01) + (wx0 * c10 + wx1 * c11) + 8) >> 4;
}

// (__mul24: the full-rate 24-bit multiply; coefficients are below 2^17 and samples below 2^14, so the low 32 bits are the product's)
template <int TOP>
__device__ __forceinline__ void to_rgb(const YuvSrc& a, int Y, int U, int V, int q[3]) {
    const int y = __mul24(a.kY, Y - a.yo), u = U - a.mid, v = V - a.mid, half = 1 << (a.T - 1);
    q[0] = clampi((y + __mul24(a.kRV, v) + half) >> a.T, 0, TOP);
    q[1] = clampi((y + __mul24(a.kGU, u) + __mul24(a.kGV, v) + half) >> a.T, 0, TOP);
    q[2] = clampi((y + __mul24(a.kBU, u) + half) >> a.T, 0, TOP);
}

// 4:2:2: the horizontal filter alone
__device__ __forceinline__ int chroma_mix_row(int c0, int c1, int wx0, int wx1) { return (wx0 * c0 + wx1 * c1 + 2) >> 2; }

// one frame pixel, every sample loaded on its own (the general path)
template <class PX, bool LEFT>
__device__ __forceinline__ void decode_pixel(const YuvSrc& a, int fy, int fx, int q[3]) {
    if constexpr (PX::SUB == 2) {               // 4:4:4: the pixel's own samples
        const long long i = (long long)fy * a.cs + fx;
        to_rgb<PX::TOP>(a, sample<PX, false>(a.yuv, (long long)fy * a.ys + fx), sample<PX, false>(a.yuv, a.uoff + i),
                        sample<PX, false>(a.yuv, a.voff + i), q);
        return;
    } else if constexpr (PX::SUB == 1) {        // 4:2:2: chroma row fy, the columns and weights of 4:2:0
        const int q0 = fx >> 1;
        const int q1 = LEFT ? min(q0 + 1, a.cw - 1) : clampi(q0 + ((fx & 1) ? 1 : -1), 0, a.cw - 1);
        const int wx0 = LEFT ? ((fx & 1) ? 2 : 4) : 3, wx1 = 4 - wx0;
        const long long i0 = (long long)fy * a.cs + q0, i1 = (long long)fy * a.cs + q1;
        const int U = chroma_mix_row(sample<PX, false>(a.yuv, a.uoff + i0), sample<PX, false>(a.yuv, a.uoff + i1), wx0, wx1);
        const int V = chroma_mix_row(sample<PX, false>(a.yuv, a.voff + i0), sample<PX, false>(a.yuv, a.voff + i1), wx0, wx1);
        to_rgb<PX::TOP>(a, sample<PX, false>(a.yuv, (long long)fy * a.ys + fx), U, V, q);
        return;
    }
    constexpr int E = PX::IL ? 2 : 1;           // samples from one chroma column to the next
    const int r0 = fy >> 1, r1 = clampi(r0 + ((fy & 1) ? 1 : -1), 0, a.ch - 1);
    const int q0 = fx >> 1;
    const int q1 = LEFT ? min(q0 + 1, a.cw - 1) : clampi(q0 + ((fx & 1) ? 1 : -1), 0, a.cw - 1);
    const int wx0 = LEFT ? ((fx & 1) ? 2 : 4) : 3, wx1 = 4 - wx0;
    const long long i00 = (long long)r0 * a.cs + E * q0, i01 = (long long)r0 * a.cs + E * q1, i10 = (long long)r1 * a.cs + E * q0,
                    i11 = (long long)r1 * a.cs + E * q1;
    const int U = chroma_mix(sample<PX, false>(a.yuv, a.uoff + i00), sample<PX, false>(a.yuv, a.uoff + i01),
                             sample<PX, false>(a.yuv, a.uoff + i10), sample<PX, false>(a.yuv, a.uoff + i11), wx0, wx1);
    const int V = chroma_mix(sample<PX, false>(a.yuv, a.voff + i00), sample<PX, false>(a.yuv, a.voff + i01),
                             sample<PX, false>(a.yuv, a.voff + i10), sample<PX, false>(a.yuv, a.voff + i11), wx0, wx1);
    to_rgb<PX::TOP>(a, sample<PX, false>(a.yuv, (long long)fy * a.ys + fx), U, V, q);
}

// four frame pixels of row fy, columns gx .. gx + 3 (gx even, the row's Y group readable as dwords) from the chroma segments of rows
// r0 / r1, seg[k] = column clamp((gx >> 1) - 1 + k) (the aligned paths).  4:2:2: u0 / v0 are the segments of chroma row fy (u1 / v1
// are not read); 4:4:4: u0 / v0 are the four samples of columns gx .. gx + 3 themselves
template <class PX, bool LEFT>
__device__ __forceinline__ void decode4(const YuvSrc& a, int fy, int gx, const int u0[4], const int u1[4], const int v0[4], const int v1[4],
                                        int q[4][3]) {
    int Y[4];
    sample_quad<PX>(a.yuv, (long long)fy * a.ys + gx, Y);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k0 = 1 + (i >> 1);
        const int k1 = LEFT ? k0 + 1 : k0 + ((i & 1) ? 1 : -1);        // (indices and weights are compile-time constants)
        const int wx0 = LEFT ? ((i & 1) ? 2 : 4) : 3, wx1 = 4 - wx0;
        int U, V;
        if constexpr (PX::SUB == 2) {
            U = u0[i];
            V = v0[i];
        } else if constexpr (PX::SUB == 1) {
            U = chroma_mix_row(u0[k0], u0[k1], wx0, wx1);
            V = chroma_mix_row(v0[k0], v0[k1], wx0, wx1);
        } else {
            U = chroma_mix(u0[k0], u0[k1], u1[k0], u1[k1], wx0, wx1);
            V = chroma_mix(v0[k0], v0[k1], v1[k0], v1[k1], wx0, wx1);
        }
        if (PX::IL) to_rgb<PX::TOP>(a, Y[i], a.vu ? V : U, a.vu ? U : V, q[i]);        // (load_row: first / second of a pair)
        else to_rgb<PX::TOP>(a, Y[i], U, V, q[i]);
    }
}

// -------------------------------------------------------------------------------------------------------------------- host: checks
// Every entry point passes its own name as the message prefix; the order of the checks is the one of atmvfi_yuv_decode (yuv.hip) and
// surface_encode (yuv_encode.hip).  They read the frame descriptor; none of these launches anything.
int check_format(const char* what, const atmvfi_yuv_desc& d) {
    const int H = d.H, W = d.W, matrix = d.matrix, full_range = d.full_range, siting = d.siting;
    ATMVFI_REQUIRE(H >= 1 && W >= 1, ATMVFI_EINVAL, "%s: H and W must be at least 1 (got %d x %d)", what, H, W);
    ATMVFI_REQUIRE(matrix == 0 || matrix == 1, ATMVFI_EINVAL, "%s: unknown matrix %d (0: bt601, 1: bt709)", what, matrix);
    ATMVFI_REQUIRE(full_range == 0 || full_range == 1, ATMVFI_EINVAL, "%s: full_range must be 0 or 1 (got %d)", what, full_range);
    ATMVFI_REQUIRE(siting == 0 || siting == 1, ATMVFI_EINVAL, "%s: unknown siting %d (0: centre, 1: left)", what, siting);
    return ATMVFI_OK;
}

int check_depth(const char* what, const atmvfi_yuv_desc& d) {
    const int depth = d.depth, full_range = d.full_range;
    ATMVFI_REQUIRE(depth == 8 || depth == 10, ATMVFI_EINVAL, "%s: depth must be 8 or 10 (got %d)", what, depth);
    ATMVFI_REQUIRE(!(depth == 10 && full_range), ATMVFI_EINVAL, "%s: 10-bit full range is not supported", what);
    return ATMVFI_OK;
}

// a surface: depth, layout and strides in BYTES as the caller gives them -> the layout in samples.  pitch / chroma_pitch / chroma_offset
// 0: tight, and so is every encode's destination (`tight`: the strides are not read).  (yuv.Surface holds the same rules.)
int check_surface(const char* what, const atmvfi_yuv_desc& d, Layout* out, bool tight = false) {
    const int H = d.H, W = d.W, depth = d.depth, chroma = d.chroma, msb = d.msb, sub = d.subsampling;
    long long pitch = tight ? 0 : d.pitch, chroma_pitch = tight ? 0 : d.chroma_pitch, chroma_offset = tight ? 0 : d.chroma_offset;
    ATMVFI_REQUIRE(chroma >= 0 && chroma <= 2, ATMVFI_EINVAL, "%s: unknown chroma layout %d (0: planar, 1: interleaved uv, 2: interleaved vu)",
                   what, chroma);
    ATMVFI_REQUIRE(msb == 0 || msb == 1, ATMVFI_EINVAL, "%s: msb must be 0 or 1 (got %d)", what, msb);
    ATMVFI_REQUIRE(!(msb && depth != 10), ATMVFI_EINVAL, "%s: msb needs depth 10 (8-bit samples fill their byte)", what);
    const long long b = depth == 10 ? 2 : 1, cw = chroma_cols(W, sub), crow = (chroma ? 2 * cw : cw) * b;
    if (pitch == 0) pitch = W * b;
    if (chroma_pitch == 0) chroma_pitch = crow;
    if (chroma_offset == 0) chroma_offset = pitch * H;
    ATMVFI_REQUIRE(pitch % b == 0 && pitch >= W * b && pitch / b < (1ll << 31), ATMVFI_EINVAL,
                   "%s: pitch %lld must be a multiple of the sample size %lld and at least a luma row's %lld bytes", what, pitch, b, W * b);
    ATMVFI_REQUIRE(chroma_pitch % b == 0 && chroma_pitch >= crow && chroma_pitch / b < (1ll << 31), ATMVFI_EINVAL,
                   "%s: chroma_pitch %lld must be a multiple of the sample size %lld and at least a chroma row's %lld bytes", what, chroma_pitch,
                   b, crow);
    ATMVFI_REQUIRE(chroma_offset % b == 0 && chroma_offset >= pitch * H, ATMVFI_EINVAL,
                   "%s: chroma_offset %lld must be a multiple of the sample size %lld and at least pitch * H = %lld", what, chroma_offset, b,
                   pitch * H);
    *out = Layout{chroma, (int)(pitch / b), (int)(chroma_pitch / b), chroma_offset / b};
    return ATMVFI_OK;
}

// 4:2:2 / 4:4:4: planar LSB frames only, no siting at 4:4:4
int check_sub(const char* what, const atmvfi_yuv_desc& d) {
    const int subsampling = d.subsampling, siting = d.siting, chroma = d.chroma, msb = d.msb;
    ATMVFI_REQUIRE(subsampling >= 0 && subsampling <= 2, ATMVFI_EINVAL, "%s: unknown subsampling %d (0: 4:2:0, 1: 4:2:2, 2: 4:4:4)", what, subsampling);
    ATMVFI_REQUIRE(subsampling == 0 || (chroma == 0 && msb == 0), ATMVFI_EINVAL,
                   "%s: 4:2:2 and 4:4:4 frames are planar with LSB samples (got chroma %d, msb %d with subsampling %d)", what, chroma, msb, subsampling);
    ATMVFI_REQUIRE(!(subsampling == 2 && siting != 0), ATMVFI_EINVAL, "%s: siting %d has no meaning for 4:4:4 (subsampling 2): give 0", what, siting);
    return ATMVFI_OK;
}

// the fp32 canvas [3,Hp,Wp] at p holds the h x w `noun` ("frame" or "window") at (pad_top, pad_left); side names the argument
int check_canvas(const char* what, const char* side, const char* noun, const float* p, int h, int w, int Hp, int Wp, int pad_top,
                 int pad_left) {
    ATMVFI_REQUIRE(aligned4(p), ATMVFI_EINVAL, "%s: %s must be 4-byte aligned", what, side);
    ATMVFI_REQUIRE(pad_top >= 0 && pad_left >= 0 && (long long)h + pad_top <= Hp && (long long)w + pad_left <= Wp, ATMVFI_EINVAL,
                   "%s: canvas %d x %d is smaller than the %s %d x %d plus padding (%d, %d)", what, Hp, Wp, noun, h, w, pad_top, pad_left);
    return ATMVFI_OK;
}

// a lane's index is an int: rows x groups work items of `thing` ("output of" the canvas, "a frame of" the encode's source)
int check_items(const char* what, long long rows, long long groups, const char* thing, int h, int w) {
    ATMVFI_REQUIRE(rows * groups < (1ll << 30), ATMVFI_EINVAL, "%s: %s %d x %d is too large", what, thing, h, w);
    return ATMVFI_OK;
}

// the frame side of the aligned paths (with a 4-byte aligned pointer and W % 4 == 0): Y groups are dwords / 8-byte words of their row,
// planar chroma pairs naturally aligned (2 or 4 bytes), interleaved chroma pair-of-pairs 4-byte aligned.  A packed I420 frame with
// W % 4 == 0 always passes.  4:4:4 (sub 2): chroma groups are loaded as Y groups are, so chroma rows are dword-aligned like luma rows.
inline bool layout_aligned(int ys, int cs, long long uoff, long long voff, const atmvfi_yuv_desc& d) {
    const int b = d.depth == 10 ? 2 : 1, sub = d.subsampling;
    const bool il = d.chroma != 0;
    if ((ys * (long long)b) % 4) return false;
    if (sub == 2) return (uoff * b) % 4 == 0 && (voff * b) % 4 == 0 && (cs * (long long)b) % 4 == 0;
    if (il) return ((uoff < voff ? uoff : voff) * b) % 4 == 0 && (cs * (long long)b) % 4 == 0;
    return uoff % 2 == 0 && voff % 2 == 0 && cs % 2 == 0;
}

inline int groups_of(int w) { return (int)(((long long)w + 3) / 4); }
inline int pairs_of(int h) { return (int)(((long long)h + 1) / 2); }

// the fp32 canvas of the aligned paths: 16-byte plane accesses, a group of four wholly inside the picture or wholly in the padding
inline bool canvas_aligned(const float* p, int Wp, int pad_left) { return atmvfi::aligned16(p) && Wp % 4 == 0 && pad_left % 4 == 0; }

// grid-stride kernels of 256 threads, at most 16 384 blocks
inline dim3 yuv_grid(long long items) {
    const long long blocks = (items + 255) / 256;
    return dim3((unsigned)(blocks > 16384 ? 16384 : blocks));
}

// run-time switches -> template parameters of a launch: dispatch(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, ...).  The siting is
// always one of them: the tap indices and weights of the chroma filter are constants of the instance.
template <class F>
void dispatch(F&& f) {
    f();
}
template <class F, class... B>
void dispatch(F&& f, bool b, B... rest) {
    if (b) dispatch([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else dispatch([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// the same with the subsampling (0, 1, 2: check_sub) as the first constant, an int
template <class F, class... B>
void dispatch_sub(F&& f, int sub, B... b) {
    if (sub == 0) dispatch([&](auto... c) { f(std::integral_constant<int, 0>{}, c...); }, b...);
    else if (sub == 1) dispatch([&](auto... c) { f(std::integral_constant<int, 1>{}, c...); }, b...);
    else dispatch([&](auto... c) { f(std::integral_constant<int, 2>{}, c...); }, b...);
}

}  // namespace
