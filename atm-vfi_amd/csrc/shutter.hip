// Synthetic shutter for the retimed video loop (include/atmvfi.h, atmvfi_shutter_accumulate / atmvfi_shutter_resolve /
// atmvfi_shutter_table; atm-vfi_amd/shutter.py holds the definition and the host twin blend_numpy).  Nothing of the reference.
//   accumulate : acc[c][y][x] (=, when first; else +=) weight * LUT[q], q the uint8 RGB pixel of one sample -- frame_f32_to_u8's pixel of
//                an fp32 canvas window, or the byte of a resident uint8 frame.  int32 planar [3,h,w], always R, G, B.
//   resolve    : v = (acc + (Wt >> 1)) / Wt, then the code whose LUT value is nearest: the number of k in 1..255 with v >= thr[k],
//                thr[k] = (LUT[k - 1] + LUT[k] + 1) >> 1, as uint8 [h,w,3].
// Integer arithmetic behind one fp32 multiply and rint: bit-exact against the loop model (tests/cpu_shutter.py) by construction.
//
// Byte-bound: per pixel 12 (fp32) or 3 (uint8) source bytes, 12 accumulator bytes written and, unless first, 12 read; resolve reads 12 and
// writes 3.  One lane owns 4 horizontally adjacent pixels:
//   aligned path: three 16-byte plane loads of the fp32 window or one 12-byte RGB group, three 16-byte accumulator accesses per
//                 direction, one 12-byte RGB store (acc and the fp32 pointer 16-byte, the byte pointers 4-byte aligned; w, Wp and
//                 pad_left multiples of 4);
//   general path: any geometry and alignment: scalar accesses, the same arithmetic.
// Grid-stride, 256 threads, every output word written by exactly one lane, no atomics, nothing pre-zeroed.  The tables sit in LDS: 256
// words filled by the block's 256 threads (the LUT for accumulate, the thresholds for resolve).  The inverse is a table read and a
// four-step search over them -- no data-dependent loop; see nearest_code -- and the division a reciprocal multiply corrected by one
// step either way (Wt is uniform; a 32-bit integer division per value would be ~25 VALU instructions, twelve times per lane).
#include "common.h"

namespace {

// LUT[light][q]: light 0 "code" = 257 q; light 1 "linear" = rint(65535 eotf(q / 255)) of the sRGB curve, float64
// (shutter.SHUTTER_TABLES; tests/test_shutter_cpu.py holds both copies to the derivation)
#define SHUTTER_LUT_CODE \
        0,   257,   514,   771,  1028,  1285,  1542,  1799,  2056,  2313,  2570,  2827,  3084,  3341,  3598,  3855, \
     4112,  4369,  4626,  4883,  5140,  5397,  5654,  5911,  6168,  6425,  6682,  6939,  7196,  7453,  7710,  7967, \
     8224,  8481,  8738,  8995,  9252,  9509,  9766, 10023, 10280, 10537, 10794, 11051, 11308, 11565, 11822, 12079, \
    12336, 12593, 12850, 13107, 13364, 13621, 13878, 14135, 14392, 14649, 14906, 15163, 15420, 15677, 15934, 16191, \
    16448, 16705, 16962, 17219, 17476, 17733, 17990, 18247, 18504, 18761, 19018, 19275, 19532, 19789, 20046, 20303, \
    20560, 20817, 21074, 21331, 21588, 21845, 22102, 22359, 22616, 22873, 23130, 23387, 23644, 23901, 24158, 24415, \
    24672, 24929, 25186, 25443, 25700, 25957, 26214, 26471, 26728, 26985, 27242, 27499, 27756, 28013, 28270, 28527, \
    28784, 29041, 29298, 29555, 29812, 30069, 30326, 30583, 30840, 31097, 31354, 31611, 31868, 32125, 32382, 32639, \
    32896, 33153, 33410, 33667, 33924, 34181, 34438, 34695, 34952, 35209, 35466, 35723, 35980, 36237, 36494, 36751, \
    37008, 37265, 37522, 37779, 38036, 38293, 38550, 38807, 39064, 39321, 39578, 39835, 40092, 40349, 40606, 40863, \
    41120, 41377, 41634, 41891, 42148, 42405, 42662, 42919, 43176, 43433, 43690, 43947, 44204, 44461, 44718, 44975, \
    45232, 45489, 45746, 46003, 46260, 46517, 46774, 47031, 47288, 47545, 47802, 48059, 48316, 48573, 48830, 49087, \
    49344, 49601, 49858, 50115, 50372, 50629, 50886, 51143, 51400, 51657, 51914, 52171, 52428, 52685, 52942, 53199, \
    53456, 53713, 53970, 54227, 54484, 54741, 54998, 55255, 55512, 55769, 56026, 56283, 56540, 56797, 57054, 57311, \
    57568, 57825, 58082, 58339, 58596, 58853, 59110, 59367, 59624, 59881, 60138, 60395, 60652, 60909, 61166, 61423, \
    61680, 61937, 62194, 62451, 62708, 62965, 63222, 63479, 63736, 63993, 64250, 64507, 64764, 65021, 65278, 65535
#define SHUTTER_LUT_LINEAR \
        0,    20,    40,    60,    80,    99,   119,   139,   159,   179,   199,   219,   241,   264,   288,   313, \
      340,   367,   396,   427,   458,   491,   526,   562,   599,   637,   677,   718,   761,   805,   851,   898, \
      947,   997,  1048,  1101,  1156,  1212,  1270,  1330,  1391,  1453,  1517,  1583,  1651,  1720,  1790,  1863, \
     1937,  2013,  2090,  2170,  2250,  2333,  2418,  2504,  2592,  2681,  2773,  2866,  2961,  3058,  3157,  3258, \
     3360,  3464,  3570,  3678,  3788,  3900,  4014,  4129,  4247,  4366,  4488,  4611,  4736,  4864,  4993,  5124, \
     5257,  5392,  5530,  5669,  5810,  5953,  6099,  6246,  6395,  6547,  6700,  6856,  7014,  7174,  7335,  7500, \
     7666,  7834,  8004,  8177,  8352,  8528,  8708,  8889,  9072,  9258,  9445,  9635,  9828, 10022, 10219, 10417, \
    10619, 10822, 11028, 11235, 11446, 11658, 11873, 12090, 12309, 12530, 12754, 12980, 13209, 13440, 13673, 13909, \
    14146, 14387, 14629, 14874, 15122, 15371, 15623, 15878, 16135, 16394, 16656, 16920, 17187, 17456, 17727, 18001, \
    18277, 18556, 18837, 19121, 19407, 19696, 19987, 20281, 20577, 20876, 21177, 21481, 21787, 22096, 22407, 22721, \
    23038, 23357, 23678, 24002, 24329, 24658, 24990, 25325, 25662, 26001, 26344, 26688, 27036, 27386, 27739, 28094, \
    28452, 28813, 29176, 29542, 29911, 30282, 30656, 31033, 31412, 31794, 32179, 32567, 32957, 33350, 33745, 34143, \
    34544, 34948, 35355, 35764, 36176, 36591, 37008, 37429, 37852, 38278, 38706, 39138, 39572, 40009, 40449, 40891, \
    41337, 41785, 42236, 42690, 43147, 43606, 44069, 44534, 45002, 45473, 45947, 46423, 46903, 47385, 47871, 48359, \
    48850, 49344, 49841, 50341, 50844, 51349, 51858, 52369, 52884, 53401, 53921, 54445, 54971, 55500, 56032, 56567, \
    57105, 57646, 58190, 58737, 59287, 59840, 60396, 60955, 61517, 62082, 62650, 63221, 63795, 64372, 64952, 65535
constexpr unsigned short kShutterLut[2][256] = {{SHUTTER_LUT_CODE}, {SHUTTER_LUT_LINEAR}};                    // atmvfi_shutter_table
__device__ const unsigned short kShutterLutDev[2][256] = {{SHUTTER_LUT_CODE}, {SHUTTER_LUT_LINEAR}};         // the kernels

typedef int i32x4 __attribute__((ext_vector_type(4)));
struct alignas(4) U32x3 {
    unsigned a, b, c;
};

struct AccumulateArgs {
    int* acc;
    int h, w, groups;           // groups = ceil(w / 4)
    const float* src;           // [3,Hp,Wp] or null
    long long src_plane;        // Hp * Wp
    int Wp, pad_top, pad_left;
    const unsigned char* u8;    // [h,w,3] or null
    int bgr, weight, light, first;
};

__device__ __forceinline__ int pixel_of(float x) {
    const int r = __float2int_rn(x * 255.0f);        // rint: half to even, as np.round (frame_f32_to_u8)
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

template <bool ALIGNED, bool F32>
__global__ __launch_bounds__(256) void shutter_accumulate_kernel(const AccumulateArgs a) {
    __shared__ int lut[256];
    lut[threadIdx.x] = kShutterLutDev[a.light][threadIdx.x];
    __syncthreads();
    const long long plane = (long long)a.h * a.w;
    const int total = a.h * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        int* o = a.acc + (long long)y * a.w + x;
        if (ALIGNED) {
            int q[3][4];        // [channel R, G, B][pixel]
            if (F32) {
                const float* p = a.src + (long long)(y + a.pad_top) * a.Wp + (x + a.pad_left);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(p + c * a.src_plane);
#pragma unroll
                    for (int i = 0; i < 4; ++i) q[c][i] = pixel_of(v[i]);
                }
            } else {
                const U32x3 r = *reinterpret_cast<const U32x3*>(a.u8 + ((long long)y * a.w + x) * 3);
                const unsigned d[3] = {r.a, r.b, r.c};
                int t[4][3];        // [pixel][byte], in source order
#pragma unroll
                for (int k = 0; k < 12; ++k) t[k / 3][k % 3] = (int)((d[k >> 2] >> ((k & 3) * 8)) & 0xffu);
#pragma unroll
                for (int i = 0; i < 4; ++i) {          // (selects, not an index computed at run time: the pixels stay in registers)
                    q[0][i] = a.bgr ? t[i][2] : t[i][0];
                    q[1][i] = t[i][1];
                    q[2][i] = a.bgr ? t[i][0] : t[i][2];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                i32x4 s = {a.weight * lut[q[c][0]], a.weight * lut[q[c][1]], a.weight * lut[q[c][2]], a.weight * lut[q[c][3]]};
                i32x4* oc = reinterpret_cast<i32x4*>(o + c * plane);
                if (!a.first) s += *oc;
                *oc = s;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.w) break;
                int q[3];
                if (F32) {
                    const float* p = a.src + (long long)(y + a.pad_top) * a.Wp + (x + i + a.pad_left);
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c] = pixel_of(p[c * a.src_plane]);
                } else {
                    const unsigned char* p = a.u8 + ((long long)y * a.w + x + i) * 3;
                    q[0] = a.bgr ? p[2] : p[0];
                    q[1] = p[1];
                    q[2] = a.bgr ? p[0] : p[2];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int s = a.weight * lut[q[c]];
                    if (!a.first) s += o[c * plane + i];
                    o[c * plane + i] = s;
                }
            }
        }
    }
}

struct ResolveArgs {
    const int* acc;
    int h, w, groups;
    int total_weight, light;
    unsigned char* u8;
    int bgr;
};

// floor((n + (Wt >> 1)) / Wt) for 0 <= n <= 65535 Wt, Wt <= 32767: the fp32 product is within 0.02 of the quotient (three roundings of
// 2^-24 on a value below 65537), so its truncation is the quotient or one beside it
__device__ __forceinline__ int rounded_mean(int n, int wt, float rcp) {
    const int t = n + (wt >> 1);
    int v = (int)((float)t * rcp);
    const int r = t - v * wt;
    v += r >= wt ? 1 : 0;
    v -= r < 0 ? 1 : 0;
    return v;
}

// The inverse: the number of k in 1..255 with v >= thr[k] (thr strictly increasing), 0 <= v <= 65535.  A plain bisection is eight
// dependent LDS reads per value whose step s reads words 2^(8 - s) apart -- all lanes on one or two banks -- and made this kernel
// instruction- and LDS-bound at 1.7 x its byte time.  Two levels instead: coarse[v >> 8] = the count for the bucket's first value, and a
// bisection of FOUR steps over the at most 15 thresholds that one bucket of 256 values can hold (static_assert below; 13 at the dark
// end of the linear table, none or one under the code table).  thr[256 .. 271] = INT_MAX ends the search without a bounds test.
// Still no data-dependent loop: one table read and four compare-and-step reads per value.
constexpr int kBucketShift = 8, kWindow = 15;
constexpr bool buckets_fit(const unsigned short (&lut)[256]) {
    int count[65536 >> kBucketShift] = {};
    for (int k = 1; k < 256; ++k) {
        if (lut[k] <= lut[k - 1]) return false;
        if (++count[((lut[k - 1] + lut[k] + 1) >> 1) >> kBucketShift] > kWindow) return false;
    }
    return true;
}
static_assert(buckets_fit(kShutterLut[0]) && buckets_fit(kShutterLut[1]), "a bucket of 256 values holds more thresholds than four steps search");

__device__ __forceinline__ int nearest_code(const int* thr, const int* coarse, int v) {
    v = (int)min((unsigned)v, 65535u);          // (an accumulator that the contract excludes must not index beyond the tables)
    int k = coarse[v >> kBucketShift];
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) k += v >= thr[k + s] ? s : 0;
    return k;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void shutter_resolve_kernel(const ResolveArgs a) {
    __shared__ int thr[256 + 16], coarse[256];
    {
        const int k = threadIdx.x;
        thr[k] = k == 0 ? 0 : ((int)kShutterLutDev[a.light][k - 1] + (int)kShutterLutDev[a.light][k] + 1) >> 1;
        if (k < 16) thr[256 + k] = 0x7fffffff;
    }
    __syncthreads();
    {       // the count for the first value of bucket b: a bisection of all eight steps, once per block
        const int v = (int)threadIdx.x << kBucketShift;
        int k = 0;
#pragma unroll
        for (int s = 128; s >= 1; s >>= 1) k += v >= thr[k + s] ? s : 0;
        coarse[threadIdx.x] = k;
    }
    __syncthreads();
    const long long plane = (long long)a.h * a.w;
    const int total = a.h * a.groups;
    const int wt = a.total_weight;
    const float rcp = 1.0f / (float)wt;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        const int* p = a.acc + (long long)y * a.w + x;
        if (ALIGNED) {
            int q[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const i32x4 s = *reinterpret_cast<const i32x4*>(p + c * plane);
#pragma unroll
                for (int i = 0; i < 4; ++i) q[c][i] = nearest_code(thr, coarse, rounded_mean(s[i], wt, rcp));
            }
            unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b0 = a.bgr ? q[2][i] : q[0][i], b2 = a.bgr ? q[0][i] : q[2][i];
                d[(3 * i) >> 2] |= (unsigned)b0 << (((3 * i) & 3) * 8);
                d[(3 * i + 1) >> 2] |= (unsigned)q[1][i] << (((3 * i + 1) & 3) * 8);
                d[(3 * i + 2) >> 2] |= (unsigned)b2 << (((3 * i + 2) & 3) * 8);
            }
            *reinterpret_cast<U32x3*>(a.u8 + ((long long)y * a.w + x) * 3) = U32x3{d[0], d[1], d[2]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.w) break;
                int q[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c] = nearest_code(thr, coarse, rounded_mean(p[c * plane + i], wt, rcp));
                unsigned char* o = a.u8 + ((long long)y * a.w + x + i) * 3;
                o[0] = (unsigned char)(a.bgr ? q[2] : q[0]);
                o[1] = (unsigned char)q[1];
                o[2] = (unsigned char)(a.bgr ? q[0] : q[2]);
            }
        }
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

inline unsigned grid_of(long long items) {
    long long b = (items + 255) / 256;
    if (b > 8192) b = 8192;      // 256 CUs x 32 blocks as the other byte-bound kernels; grid-stride the rest
    return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" int atmvfi_shutter_accumulate(int32_t* acc, int h, int w, const float* src, int Hp, int Wp, int pad_top, int pad_left,
                                          const uint8_t* src_u8, int bgr, int weight, int light, int first, void* stream) {
    ATMVFI_REQUIRE(acc, ATMVFI_EINVAL, "shutter_accumulate: null accumulator");
    ATMVFI_REQUIRE((src != nullptr) != (src_u8 != nullptr), ATMVFI_EINVAL, "shutter_accumulate: give exactly one of src and src_u8");
    ATMVFI_REQUIRE(h >= 1 && w >= 1, ATMVFI_EINVAL, "shutter_accumulate: negative or zero size (%d x %d)", h, w);
    ATMVFI_REQUIRE(!src || (Hp >= 1 && Wp >= 1 && pad_top >= 0 && pad_left >= 0 && (long long)pad_top + h <= Hp && (long long)pad_left + w <= Wp),
                   ATMVFI_EINVAL, "shutter_accumulate: window outside the canvas (%d x %d at (%d, %d) of %d x %d)", h, w, pad_top, pad_left, Hp,
                   Wp);
    ATMVFI_REQUIRE(weight >= 1 && weight <= 32767, ATMVFI_EINVAL, "shutter_accumulate: weight %d outside 1..32767", weight);
    ATMVFI_REQUIRE(light == 0 || light == 1, ATMVFI_EINVAL, "shutter_accumulate: unknown light %d (0: code, 1: linear)", light);
    ATMVFI_REQUIRE(aligned4(acc) && (!src || aligned4(src)), ATMVFI_EINVAL, "shutter_accumulate: acc and src must be 4-byte aligned");
    const int groups = (int)(((long long)w + 3) / 4);
    ATMVFI_REQUIRE((long long)h * groups < (1ll << 30) && (!src || (long long)Hp * Wp < (1ll << 31)), ATMVFI_EINVAL,
                   "shutter_accumulate: a frame of %d x %d is too large (the work-item count must fit an int)", h, w);
    const AccumulateArgs a = {acc, h, w, groups, src, (long long)Hp * Wp, Wp, pad_top, pad_left, src_u8, bgr ? 1 : 0, weight, light, first ? 1 : 0};
    const dim3 grid(grid_of((long long)h * groups)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (src) {
        const bool al = atmvfi::aligned16(acc) && atmvfi::aligned16(src) && w % 4 == 0 && Wp % 4 == 0 && pad_left % 4 == 0;
        if (al) hipLaunchKernelGGL((shutter_accumulate_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((shutter_accumulate_kernel<false, true>), grid, block, 0, st, a);
    } else {
        const bool al = atmvfi::aligned16(acc) && aligned4(src_u8) && w % 4 == 0;
        if (al) hipLaunchKernelGGL((shutter_accumulate_kernel<true, false>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((shutter_accumulate_kernel<false, false>), grid, block, 0, st, a);
    }
    return atmvfi::check_launch("shutter_accumulate");
}

extern "C" int atmvfi_shutter_resolve(const int32_t* acc, int h, int w, int total_weight, int light, uint8_t* dst_u8, int bgr, void* stream) {
    ATMVFI_REQUIRE(acc && dst_u8, ATMVFI_EINVAL, "shutter_resolve: null pointer (acc %p, dst_u8 %p)", (const void*)acc, (void*)dst_u8);
    ATMVFI_REQUIRE(h >= 1 && w >= 1, ATMVFI_EINVAL, "shutter_resolve: negative or zero size (%d x %d)", h, w);
    ATMVFI_REQUIRE(total_weight >= 1 && total_weight <= 32767, ATMVFI_EINVAL, "shutter_resolve: total_weight %d outside 1..32767", total_weight);
    ATMVFI_REQUIRE(light == 0 || light == 1, ATMVFI_EINVAL, "shutter_resolve: unknown light %d (0: code, 1: linear)", light);
    ATMVFI_REQUIRE(aligned4(acc), ATMVFI_EINVAL, "shutter_resolve: acc must be 4-byte aligned");
    const int groups = (int)(((long long)w + 3) / 4);
    ATMVFI_REQUIRE((long long)h * groups < (1ll << 30), ATMVFI_EINVAL,
                   "shutter_resolve: a frame of %d x %d is too large (the work-item count must fit an int)", h, w);
    const ResolveArgs a = {acc, h, w, groups, total_weight, light, dst_u8, bgr ? 1 : 0};
    const dim3 grid(grid_of((long long)h * groups)), block(256);
    const bool al = atmvfi::aligned16(acc) && aligned4(dst_u8) && w % 4 == 0;
    if (al) hipLaunchKernelGGL((shutter_resolve_kernel<true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((shutter_resolve_kernel<false>), grid, block, 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("shutter_resolve");
}

extern "C" int atmvfi_shutter_table(int light, uint16_t out[256]) {
    ATMVFI_REQUIRE(out, ATMVFI_EINVAL, "shutter_table: null output");
    ATMVFI_REQUIRE(light == 0 || light == 1, ATMVFI_EINVAL, "shutter_table: unknown light %d (0: code, 1: linear)", light);
    for (int q = 0; q < 256; ++q) out[q] = kShutterLut[light][q];
    return ATMVFI_OK;
}
