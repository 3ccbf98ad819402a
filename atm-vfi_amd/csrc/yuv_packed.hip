// Packed 4:2:2 capture frames <-> the tight planar 4:2:2 frame (include/atmvfi.h, atmvfi_yuv_unpack / atmvfi_yuv_pack; atm-vfi_amd/pixfmt.py
// Packed holds the layouts, yuv.unpack_numpy / pack_numpy are the host twins, tests/cpu_yuv_packed.py the per-sample model).  Nothing of
// the reference.  Sample-exact: shifts and masks only.
//   layout 0 uyvy : uint8            U0 Y0 V0 Y1 per pixel pair
//   layout 1 yuy2 : uint8            Y0 U0 Y1 V0
//   layout 2 y210 : uint16 (LE)      Y0 U0 Y1 V0, a sample is value << 6
//   layout 3 v210 : four LE dwords per 6 pixels, three 10-bit components each (bits 0-9, 10-19, 20-29):
//                   w0 = (Cb0, Y0, Cr0)  w1 = (Y1, Cb1, Y2)  w2 = (Cr1, Y3, Cb2)  w3 = (Y4, Cr2, Y5)
// planar: Y [H,W], U [H,W/2], V [H,W/2] back to back, uint8 or LSB-aligned uint16: what atmvfi_yuv_decode / atmvfi_yuv_encode (subsampling 1) read and write.
//
// Byte-bound: per pixel 2 (8 bit), 4 (y210) or 8/3 (v210) packed bytes on one side and 2 or 4 planar bytes on the other.  Items:
//   layouts 0-2: an item is 32 packed bytes of one row (16 pixels at 8 bit, 8 at y210).  Aligned path (both pointers 16-byte aligned, the
//                pitch a multiple of 16, W a multiple of the item's pixels): two 16-byte accesses of the packed row, one 16-byte access
//                of the luma row and one 8-byte access per chroma row.  General path: any W, pitch and sample-aligned pointers, sample
//                accesses, the same moves.
//   v210:        the leading `quads` items of a row are FOUR whole groups (64 packed bytes, 24 pixels): four 16-byte accesses of the packed
//                row, three 16-byte accesses of the luma row, three 8-byte accesses per chroma row (both pointers 16-byte aligned, W a
//                multiple of 8; else quads = 0).  Every further item is ONE group through dword accesses of the packed row (always 4-byte
//                aligned) and sample accesses of the planes: the groups behind the last whole quad, the partial last group, and -- pack
//                only -- the all-zero groups of the row's padding up to the default pitch.
// Unpack reads a row's groups only (never beyond ceil(W / 6) * 16 or 2 W b bytes of a row) and writes every planar sample; pack reads
// the planes only and writes every byte of the default-pitch frame: unused component slots, bits 30-31, y210's low six bits and the
// row padding as zero.  Grid-stride, 256 threads, every output byte written by exactly one lane, vector stores only, no atomics, nothing
// pre-zeroed, no LDS.
#include "common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct PackedArgs {
    unsigned char* packed;
    unsigned char* planar;
    int H, W;
    long long pitch;        // of the packed rows, bytes
    int items;              // per row
    int quads;              // v210: the leading items of a row that are four whole groups
    int groups;             // v210: the groups of a row that hold samples, ceil(W / 6)
};

// ---------------------------------------------------------------------------------------------------- uyvy, yuy2, y210
template <int LAYOUT>
struct Lay {
    typedef typename std::conditional<LAYOUT == 2, unsigned short, unsigned char>::type T;
    static constexpr int B = (int)sizeof(T);        // bytes per sample
    static constexpr int SB = 8 * B;                // bits per sample
    static constexpr int PAIRS = 8 / B;             // pixel pairs of an item (32 packed bytes)
    static constexpr int SHIFT = LAYOUT == 2 ? 6 : 0;
    static constexpr unsigned MASK = LAYOUT == 2 ? 0xffffu : 0xffu;
    // sample slots of a pair, in memory order
    static constexpr int Y0 = LAYOUT == 0 ? 1 : 0, U = LAYOUT == 0 ? 0 : 1, Y1 = LAYOUT == 0 ? 3 : 2, V = LAYOUT == 0 ? 2 : 3;
};

// sample `slot` (0..3) of pair k among the item's eight dwords, as stored
template <int LAYOUT>
__device__ __forceinline__ unsigned stored_sample(const unsigned (&d)[8], int k, int slot) {
    constexpr int SB = Lay<LAYOUT>::SB;
    const int bit = (4 * k + slot) * SB;
    return (d[bit >> 5] >> (bit & 31)) & Lay<LAYOUT>::MASK;
}

template <int LAYOUT, bool ALIGNED, bool PACK>
__global__ __launch_bounds__(256) void yuv_packed_pairs_kernel(const PackedArgs a) {
    typedef Lay<LAYOUT> L;
    typedef typename L::T T;
    constexpr int PAIRS = L::PAIRS, SB = L::SB, SHIFT = L::SHIFT;
    const int cw = a.W >> 1;
    const long long luma = (long long)a.H * a.W, chroma = (long long)a.H * cw;
    const int total = a.H * a.items;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.items, x = (idx - y * a.items) * (2 * PAIRS);
        unsigned char* prow = a.packed + (long long)y * a.pitch + (long long)x * 2 * L::B;
        T* Yp = reinterpret_cast<T*>(a.planar) + (long long)y * a.W + x;
        T* Up = reinterpret_cast<T*>(a.planar) + luma + (long long)y * cw + (x >> 1);
        T* Vp = Up + chroma;
        if (ALIGNED) {
            unsigned d[8], Yw[4], Uw[2], Vw[2];
            if (!PACK) {
                const u32x4 p0 = reinterpret_cast<const u32x4*>(prow)[0], p1 = reinterpret_cast<const u32x4*>(prow)[1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    d[i] = p0[i];
                    d[4 + i] = p1[i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) Yw[i] = 0u;
                Uw[0] = Uw[1] = Vw[0] = Vw[1] = 0u;
#pragma unroll
                for (int k = 0; k < PAIRS; ++k) {
                    const unsigned y0 = stored_sample<LAYOUT>(d, k, L::Y0) >> SHIFT, y1 = stored_sample<LAYOUT>(d, k, L::Y1) >> SHIFT;
                    const unsigned u = stored_sample<LAYOUT>(d, k, L::U) >> SHIFT, v = stored_sample<LAYOUT>(d, k, L::V) >> SHIFT;
                    Yw[(2 * k * SB) >> 5] |= y0 << ((2 * k * SB) & 31);
                    Yw[((2 * k + 1) * SB) >> 5] |= y1 << (((2 * k + 1) * SB) & 31);
                    Uw[(k * SB) >> 5] |= u << ((k * SB) & 31);
                    Vw[(k * SB) >> 5] |= v << ((k * SB) & 31);
                }
                *reinterpret_cast<u32x4*>(Yp) = u32x4{Yw[0], Yw[1], Yw[2], Yw[3]};
                *reinterpret_cast<u32x2*>(Up) = u32x2{Uw[0], Uw[1]};
                *reinterpret_cast<u32x2*>(Vp) = u32x2{Vw[0], Vw[1]};
            } else {
                const u32x4 yv = *reinterpret_cast<const u32x4*>(Yp);
                const u32x2 uv = *reinterpret_cast<const u32x2*>(Up), vv = *reinterpret_cast<const u32x2*>(Vp);
#pragma unroll
                for (int i = 0; i < 4; ++i) Yw[i] = yv[i];
                Uw[0] = uv[0], Uw[1] = uv[1], Vw[0] = vv[0], Vw[1] = vv[1];
#pragma unroll
                for (int i = 0; i < 8; ++i) d[i] = 0u;
#pragma unroll
                for (int k = 0; k < PAIRS; ++k) {
                    unsigned s[4];
                    s[L::Y0] = (Yw[(2 * k * SB) >> 5] >> ((2 * k * SB) & 31)) & L::MASK;
                    s[L::Y1] = (Yw[((2 * k + 1) * SB) >> 5] >> (((2 * k + 1) * SB) & 31)) & L::MASK;
                    s[L::U] = (Uw[(k * SB) >> 5] >> ((k * SB) & 31)) & L::MASK;
                    s[L::V] = (Vw[(k * SB) >> 5] >> ((k * SB) & 31)) & L::MASK;
#pragma unroll
                    for (int slot = 0; slot < 4; ++slot) {
                        const int bit = (4 * k + slot) * SB;
                        d[bit >> 5] |= ((s[slot] << SHIFT) & L::MASK) << (bit & 31);
                    }
                }
                reinterpret_cast<u32x4*>(prow)[0] = u32x4{d[0], d[1], d[2], d[3]};
                reinterpret_cast<u32x4*>(prow)[1] = u32x4{d[4], d[5], d[6], d[7]};
            }
        } else {
            T* s = reinterpret_cast<T*>(prow);
#pragma unroll
            for (int k = 0; k < PAIRS; ++k) {
                if (x + 2 * k >= a.W) break;        // (W is even: a pair is whole)
                if (!PACK) {
                    Yp[2 * k] = (T)(s[4 * k + L::Y0] >> SHIFT);
                    Yp[2 * k + 1] = (T)(s[4 * k + L::Y1] >> SHIFT);
                    Up[k] = (T)(s[4 * k + L::U] >> SHIFT);
                    Vp[k] = (T)(s[4 * k + L::V] >> SHIFT);
                } else {
                    s[4 * k + L::Y0] = (T)((unsigned)Yp[2 * k] << SHIFT);
                    s[4 * k + L::Y1] = (T)((unsigned)Yp[2 * k + 1] << SHIFT);
                    s[4 * k + L::U] = (T)((unsigned)Up[k] << SHIFT);
                    s[4 * k + L::V] = (T)((unsigned)Vp[k] << SHIFT);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- v210
__device__ __forceinline__ void v210_decode(const unsigned (&w)[4], unsigned (&y)[6], unsigned (&cb)[3], unsigned (&cr)[3]) {
    cb[0] = w[0] & 0x3ffu, y[0] = (w[0] >> 10) & 0x3ffu, cr[0] = (w[0] >> 20) & 0x3ffu;
    y[1] = w[1] & 0x3ffu, cb[1] = (w[1] >> 10) & 0x3ffu, y[2] = (w[1] >> 20) & 0x3ffu;
    cr[1] = w[2] & 0x3ffu, y[3] = (w[2] >> 10) & 0x3ffu, cb[2] = (w[2] >> 20) & 0x3ffu;
    y[4] = w[3] & 0x3ffu, cr[2] = (w[3] >> 10) & 0x3ffu, y[5] = (w[3] >> 20) & 0x3ffu;
}

__device__ __forceinline__ void v210_encode(const unsigned (&y)[6], const unsigned (&cb)[3], const unsigned (&cr)[3], unsigned (&w)[4]) {
    w[0] = (cb[0] & 0x3ffu) | (y[0] & 0x3ffu) << 10 | (cr[0] & 0x3ffu) << 20;
    w[1] = (y[1] & 0x3ffu) | (cb[1] & 0x3ffu) << 10 | (y[2] & 0x3ffu) << 20;
    w[2] = (cr[1] & 0x3ffu) | (y[3] & 0x3ffu) << 10 | (cb[2] & 0x3ffu) << 20;
    w[3] = (y[4] & 0x3ffu) | (cr[2] & 0x3ffu) << 10 | (y[5] & 0x3ffu) << 20;
}

template <bool PACK>
__global__ __launch_bounds__(256) void yuv_packed_v210_kernel(const PackedArgs a) {
    const int cw = a.W >> 1;
    const long long luma = (long long)a.H * a.W, chroma = (long long)a.H * cw;
    const int total = a.H * a.items;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.items, j = idx - y * a.items;
        unsigned char* prow = a.packed + (long long)y * a.pitch;
        unsigned short* Yr = reinterpret_cast<unsigned short*>(a.planar) + (long long)y * a.W;
        unsigned short* Ur = reinterpret_cast<unsigned short*>(a.planar) + luma + (long long)y * cw;
        unsigned short* Vr = Ur + chroma;
        if (j < a.quads) {                  // four whole groups: pixels 24 j .. 24 j + 23
            u32x4* p = reinterpret_cast<u32x4*>(prow) + 4 * j;
            u32x4* Yp = reinterpret_cast<u32x4*>(Yr + 24 * j);
            u32x2* Up = reinterpret_cast<u32x2*>(Ur + 12 * j);
            u32x2* Vp = reinterpret_cast<u32x2*>(Vr + 12 * j);
            unsigned yy[24], cb[12], cr[12];
            if (!PACK) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const u32x4 g = p[t];
                    const unsigned w[4] = {g[0], g[1], g[2], g[3]};
                    unsigned y6[6], b3[3], r3[3];
                    v210_decode(w, y6, b3, r3);
#pragma unroll
                    for (int i = 0; i < 6; ++i) yy[6 * t + i] = y6[i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) cb[3 * t + i] = b3[i], cr[3 * t + i] = r3[i];
                }
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    Yp[t] = u32x4{yy[8 * t] | yy[8 * t + 1] << 16, yy[8 * t + 2] | yy[8 * t + 3] << 16, yy[8 * t + 4] | yy[8 * t + 5] << 16,
                                  yy[8 * t + 6] | yy[8 * t + 7] << 16};
                    Up[t] = u32x2{cb[4 * t] | cb[4 * t + 1] << 16, cb[4 * t + 2] | cb[4 * t + 3] << 16};
                    Vp[t] = u32x2{cr[4 * t] | cr[4 * t + 1] << 16, cr[4 * t + 2] | cr[4 * t + 3] << 16};
                }
            } else {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const u32x4 yv = Yp[t];
                    const u32x2 uv = Up[t], vv = Vp[t];
#pragma unroll
                    for (int i = 0; i < 4; ++i) yy[8 * t + 2 * i] = yv[i] & 0xffffu, yy[8 * t + 2 * i + 1] = yv[i] >> 16;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        cb[4 * t + 2 * i] = uv[i] & 0xffffu, cb[4 * t + 2 * i + 1] = uv[i] >> 16;
                        cr[4 * t + 2 * i] = vv[i] & 0xffffu, cr[4 * t + 2 * i + 1] = vv[i] >> 16;
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    unsigned y6[6], b3[3], r3[3], w[4];
#pragma unroll
                    for (int i = 0; i < 6; ++i) y6[i] = yy[6 * t + i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) b3[i] = cb[3 * t + i], r3[i] = cr[3 * t + i];
                    v210_encode(y6, b3, r3, w);
                    p[t] = u32x4{w[0], w[1], w[2], w[3]};
                }
            }
        } else {                            // one group: pixels 6 g .. 6 g + 5 as far as the row has them
            const int g = 4 * a.quads + (j - a.quads), px = 6 * g, cx = 3 * g;
            unsigned* p = reinterpret_cast<unsigned*>(prow) + 4 * g;
            unsigned w[4], y6[6], b3[3], r3[3];
            if (!PACK) {
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = p[i];
                v210_decode(w, y6, b3, r3);
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    if (px + i < a.W) Yr[px + i] = (unsigned short)y6[i];
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (cx + i < cw) Ur[cx + i] = (unsigned short)b3[i], Vr[cx + i] = (unsigned short)r3[i];
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i) y6[i] = (g < a.groups && px + i < a.W) ? Yr[px + i] : 0u;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const bool in = g < a.groups && cx + i < cw;
                    b3[i] = in ? Ur[cx + i] : 0u;
                    r3[i] = in ? Vr[cx + i] : 0u;
                }
                v210_encode(y6, b3, r3, w);
#pragma unroll
                for (int i = 0; i < 4; ++i) p[i] = w[i];
            }
        }
    }
}

inline unsigned grid_of(long long items) {
    long long b = (items + 255) / 256;
    if (b > 8192) b = 8192;      // 256 CUs x 32 blocks as the other byte-bound kernels; grid-stride the rest
    return (unsigned)(b < 1 ? 1 : b);
}

inline bool aligned_to(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) == 0; }

const char* const kLayoutNames[4] = {"uyvy", "yuy2", "y210", "v210"};

template <int LAYOUT, bool PACK>
void launch_pairs(bool aligned, dim3 grid, hipStream_t st, const PackedArgs& a) {
    if (aligned) hipLaunchKernelGGL((yuv_packed_pairs_kernel<LAYOUT, true, PACK>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((yuv_packed_pairs_kernel<LAYOUT, false, PACK>), grid, dim3(256), 0, st, a);
}

// The one checked host path of both directions: `pitch` 0 is the default pitch (pack always writes it).
template <bool PACK>
int packed_call(const char* who, const void* packed, const void* planar, int H, int W, int layout, long long pitch, void* stream) {
    ATMVFI_REQUIRE(packed && planar, ATMVFI_EINVAL, "%s: null pointer (packed %p, planar %p)", who, packed, planar);
    ATMVFI_REQUIRE(layout >= 0 && layout <= 3, ATMVFI_EINVAL, "%s: unknown layout %d (0: uyvy, 1: yuy2, 2: y210, 3: v210)", who, layout);
    ATMVFI_REQUIRE(H >= 1 && W >= 2 && W % 2 == 0, ATMVFI_EINVAL, "%s: %d x %d: H must be at least 1 and W even and at least 2 (%s carries chroma per pixel pair)",
                   who, H, W, kLayoutNames[layout]);
    const int b = layout >= 2 ? 2 : 1;              // bytes per planar sample
    const long long groups = ((long long)W + 5) / 6;
    const long long row = layout == 3 ? groups * 16 : (long long)W * 2 * b;
    const long long tight = layout == 3 ? (((long long)W + 47) / 48) * 128 : row;
    const long long unit = layout == 3 ? 16 : 4;
    if (pitch == 0) pitch = tight;
    ATMVFI_REQUIRE(pitch >= row && pitch % unit == 0, ATMVFI_EINVAL, "%s: pitch %lld must be a multiple of %lld and at least a %s row's %lld bytes", who,
                   pitch, unit, kLayoutNames[layout], row);
    const unsigned pa = layout == 3 ? 4u : (unsigned)b;
    ATMVFI_REQUIRE(aligned_to(packed, pa) && aligned_to(planar, (unsigned)b), ATMVFI_EINVAL,
                   "%s: a %s frame must be %u-byte aligned and its planar frame %d-byte aligned (packed %p, planar %p)", who, kLayoutNames[layout], pa, b,
                   packed, planar);
    const long long planar_bytes = (long long)H * W * 2 * b, packed_bytes = pitch * (H - 1) + (PACK ? pitch : row);
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(packed), q0 = reinterpret_cast<uintptr_t>(planar);
    ATMVFI_REQUIRE(p0 + (uintptr_t)packed_bytes <= q0 || q0 + (uintptr_t)planar_bytes <= p0, ATMVFI_EINVAL, "%s: packed and planar overlap", who);
    PackedArgs a = {(unsigned char*)packed, (unsigned char*)planar, H, W, pitch, 0, 0, (int)groups};
    const bool al16 = atmvfi::aligned16(packed) && atmvfi::aligned16(planar) && pitch % 16 == 0;
    long long items;
    if (layout == 3) {
        a.quads = (al16 && W % 8 == 0) ? (W / 6) / 4 : 0;
        items = a.quads + ((PACK ? pitch / 16 : groups) - 4ll * a.quads);
    } else {
        items = ((long long)W + 16 / b - 1) / (16 / b);
    }
    ATMVFI_REQUIRE((long long)H * items < (1ll << 30), ATMVFI_EINVAL, "%s: a frame of %d x %d is too large (the work-item count must fit an int)", who, H,
                   W);
    a.items = (int)items;
    const dim3 grid(grid_of((long long)H * items));
    const hipStream_t st = (hipStream_t)stream;
    const bool aligned = al16 && W % (16 / b) == 0;
    switch (layout) {
        case 0: launch_pairs<0, PACK>(aligned, grid, st, a); break;
        case 1: launch_pairs<1, PACK>(aligned, grid, st, a); break;
        case 2: launch_pairs<2, PACK>(aligned, grid, st, a); break;
        default: hipLaunchKernelGGL((yuv_packed_v210_kernel<PACK>), grid, dim3(256), 0, st, a); break;
    }
    return atmvfi::check_launch(who);
}

}  // namespace

extern "C" int atmvfi_yuv_unpack(const void* packed, int H, int W, int layout, int64_t pitch, void* planar, void* stream) {
    ATMVFI_REQUIRE(pitch >= 0, ATMVFI_EINVAL, "yuv_unpack: negative pitch %lld", (long long)pitch);
    return packed_call<false>("yuv_unpack", packed, planar, H, W, layout, (long long)pitch, stream);
}

extern "C" int atmvfi_yuv_pack(const void* planar, int H, int W, int layout, void* packed, void* stream) {
    return packed_call<true>("yuv_pack", packed, planar, H, W, layout, 0, stream);
}
