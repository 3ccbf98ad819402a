// Multi-frame (4x / 8x recursive) interpolation: the data movement around the forward (include/atmvfi.h, atmvfi_pool_blocks,
// atmvfi_tta_merge, atmvfi_frame_rot180; benchmark/davis-vid.py:98-135 of the reference).
//   pool_blocks : n blocks between the slots of a frame / token pool and one contiguous buffer, either direction, ONE launch.  The slot
//                 list is a host array read at call time; it travels in the kernel arguments (no device table, no copy, capturable).
//   tta_merge   : out = (pred + rot180(pred_flip)) / 2 in fp32 and / or its uint8 [H,W,3] form (crop, x * 255, round half to even,
//                 optional RGB -> BGR): the flip-TTA tail (flip, flip, add, divide, convert) in one pass.
//   frame_rot180: flip(H).flip(W) of C contiguous planes = the flattened reversal of each plane (same kernel, a template flag).
//
// All three are bandwidth-bound and small.  Bytes (read + written) at 1080p padded to 1088x1920 (one fp32 frame = 25.1 MB):
//   pool_blocks  2 x block_bytes per block: a frame 25.1 MB, its local tokens (base: 32640 x 384 fp32) 50.1 MB, its global tokens
//                (8160 x 672) 21.9 MB; the three gathers of a batch of 4 pairs move 2 x 8 x 97.1 MB = 1.55 GB
//   tta_merge    2 x 25.1 MB in, 25.1 MB (fp32) + 6.2 MB (uint8) out
//   frame_rot180 25.1 MB in, 25.1 MB out
// 16 bytes per lane on every fp32 access (plain loads and stores: what is gathered is read by the very next launch, and plain stores keep
// the lines in L2); the reversed operand is read backwards with 16-byte loads and a lane-local swizzle (w, z, y, x) -- no second pass,
// no transposition.  A scalar path takes planes whose size is no multiple of 4 or whose pointers are not 16-byte aligned; same bits.
#include "common.h"

namespace {

constexpr int kMaxBlocks = 32;

struct PoolArgs {
    char* pool;
    char* buf;
    long long slot_bytes;
    long long vecs;             // block_bytes / 16
    int slots[kMaxBlocks];
};

template <bool TO_POOL>
__global__ __launch_bounds__(256) void pool_blocks_kernel(const PoolArgs a) {
    const int j = blockIdx.y;
    f32x4* p = reinterpret_cast<f32x4*>(a.pool + (long long)a.slots[j] * a.slot_bytes);
    f32x4* b = reinterpret_cast<f32x4*>(a.buf + (long long)j * a.vecs * 16);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.vecs; i += (long long)gridDim.x * blockDim.x) {
        if (TO_POOL) p[i] = b[i];
        else b[i] = p[i];
    }
}

struct MergeArgs {
    const float* pred;          // null with ROT_ONLY
    const float* flip;
    float* out;
    unsigned char* u8;
    int C;
    long long plane;            // Hp * Wp
    int Hp, Wp, pad_top, pad_left, H, W, bgr;
};

template <bool VEC>
struct Group;
template <>
struct Group<true> {
    typedef f32x4 T;
    static constexpr int N = 4;
    static __device__ __forceinline__ T load(const float* base, long long g) { return *reinterpret_cast<const f32x4*>(base + 4 * g); }
    // elements plane-1-4g, plane-2-4g, ...: the group that ends at plane - 4g, reversed inside the lane
    static __device__ __forceinline__ T load_rev(const float* base, long long plane, long long g) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(base + plane - 4 - 4 * g);
        return (f32x4){t.w, t.z, t.y, t.x};
    }
    static __device__ __forceinline__ void store(float* base, long long g, T v) { *reinterpret_cast<f32x4*>(base + 4 * g) = v; }
    static __device__ __forceinline__ float at(T v, int i) { return v[i]; }
};
template <>
struct Group<false> {
    typedef float T;
    static constexpr int N = 1;
    static __device__ __forceinline__ T load(const float* base, long long g) { return base[g]; }
    static __device__ __forceinline__ T load_rev(const float* base, long long plane, long long g) { return base[plane - 1 - g]; }
    static __device__ __forceinline__ void store(float* base, long long g, T v) { base[g] = v; }
    static __device__ __forceinline__ float at(T v, int) { return v; }
};

template <bool VEC, bool ROT_ONLY>
__global__ __launch_bounds__(256) void tta_merge_kernel(const MergeArgs a) {
    typedef Group<VEC> G;
    const long long groups = a.plane / G::N;
    const long long total = ROT_ONLY ? groups * a.C : groups;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        if (ROT_ONLY) {
            const long long c = idx / groups, g = idx - c * groups;
            G::store(a.out + c * a.plane, g, G::load_rev(a.flip + c * a.plane, a.plane, g));
        } else {
            typename G::T v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = (G::load(a.pred + c * a.plane, idx) + G::load_rev(a.flip + c * a.plane, a.plane, idx)) / 2.0f;
                if (a.out) G::store(a.out + c * a.plane, idx, v[c]);
            }
            if (a.u8) {
#pragma unroll
                for (int i = 0; i < G::N; ++i) {
                    const long long pix = idx * G::N + i;
                    const int yy = (int)(pix / a.Wp);
                    const int y = yy - a.pad_top, x = (int)(pix - (long long)yy * a.Wp) - a.pad_left;
                    if (y < 0 || y >= a.H || x < 0 || x >= a.W) continue;
                    int q[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int r = __float2int_rn(G::at(v[c], i) * 255.0f);        // rint: half to even, as np.round (frame_f32_to_u8)
                        q[c] = r < 0 ? 0 : (r > 255 ? 255 : r);
                    }
                    unsigned char* o = a.u8 + ((long long)y * a.W + x) * 3;
                    o[0] = (unsigned char)(a.bgr ? q[2] : q[0]);
                    o[1] = (unsigned char)q[1];
                    o[2] = (unsigned char)(a.bgr ? q[0] : q[2]);
                }
            }
        }
    }
}

inline unsigned capped_grid(long long items, long long cap) {
    long long b = (items + 255) / 256;
    if (b > cap) b = cap;      // 256 CUs x 32 blocks as the other pointwise kernels; grid-stride the rest
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

extern "C" int atmvfi_pool_blocks(void* pool, int64_t slot_bytes, int n_slots, const int32_t* slots, int n, int64_t block_bytes, void* buf,
                                   int to_pool, void* stream) {
    ATMVFI_REQUIRE(pool && buf, ATMVFI_EINVAL, "pool_blocks: null pool or buffer");
    ATMVFI_REQUIRE(slots, ATMVFI_EINVAL, "pool_blocks: null slot list");
    ATMVFI_REQUIRE(n >= 1 && n <= kMaxBlocks, ATMVFI_EINVAL, "pool_blocks: n %d outside 1..%d", n, kMaxBlocks);
    ATMVFI_REQUIRE(n_slots >= 1 && slot_bytes > 0 && slot_bytes % 16 == 0, ATMVFI_EINVAL,
                   "pool_blocks: bad pool geometry (%d slots of %lld bytes; slot_bytes must be a positive multiple of 16)", n_slots,
                   (long long)slot_bytes);
    ATMVFI_REQUIRE(block_bytes > 0 && block_bytes <= slot_bytes && block_bytes % 16 == 0, ATMVFI_EINVAL,
                   "pool_blocks: block_bytes %lld must be a multiple of 16 in 16..slot_bytes (%lld)", (long long)block_bytes,
                   (long long)slot_bytes);
    ATMVFI_REQUIRE(atmvfi::aligned16(pool) && atmvfi::aligned16(buf), ATMVFI_EINVAL, "pool_blocks: pool and buffer must be 16-byte aligned");
    PoolArgs a;
    a.pool = (char*)pool;
    a.buf = (char*)buf;
    a.slot_bytes = slot_bytes;
    a.vecs = block_bytes / 16;
    unsigned seen_lo = 0;       // slots 0..31 as a bit mask, larger ones pairwise: scatter must not name a slot twice
    for (int j = 0; j < kMaxBlocks; ++j) a.slots[j] = 0;
    for (int j = 0; j < n; ++j) {
        const int s = slots[j];
        ATMVFI_REQUIRE(s >= 0 && s < n_slots, ATMVFI_EINVAL, "pool_blocks: slot %d (entry %d) outside 0..%d", s, j, n_slots - 1);
        if (to_pool) {
            bool dup = s < 32 ? ((seen_lo >> s) & 1u) != 0 : false;
            if (s < 32) seen_lo |= 1u << s;
            else
                for (int k = 0; k < j; ++k) dup = dup || slots[k] == s;
            ATMVFI_REQUIRE(!dup, ATMVFI_EINVAL, "pool_blocks: scatter names slot %d twice", s);
        }
        a.slots[j] = s;
    }
    const long long cap = 8192 / n;
    const dim3 grid(capped_grid(a.vecs, cap < 1 ? 1 : cap), (unsigned)n), block(256);
    if (to_pool) hipLaunchKernelGGL(pool_blocks_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(pool_blocks_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("pool_blocks");
}

extern "C" int atmvfi_tta_merge(const float* pred, const float* pred_flip, float* out, void* out_u8, int Hp, int Wp, int pad_top, int pad_left,
                                 int H, int W, int bgr, void* stream) {
    ATMVFI_REQUIRE(pred && pred_flip, ATMVFI_EINVAL, "tta_merge: null prediction");
    ATMVFI_REQUIRE(out || out_u8, ATMVFI_EINVAL, "tta_merge: both outputs are null (give out, out_u8 or both)");
    ATMVFI_REQUIRE(Hp > 0 && Wp > 0 && (long long)Hp * Wp < (1ll << 31), ATMVFI_EINVAL, "tta_merge: bad canvas %d x %d", Hp, Wp);
    ATMVFI_REQUIRE(!out_u8 || (H > 0 && W > 0 && pad_top >= 0 && pad_left >= 0 && (long long)pad_top + H <= Hp && (long long)pad_left + W <= Wp),
                   ATMVFI_EINVAL, "tta_merge: bad geometry (Hp %d Wp %d -> H %d W %d, pad %d %d)", Hp, Wp, H, W, pad_top, pad_left);
    const long long plane = (long long)Hp * Wp;
    const MergeArgs a = {pred, pred_flip, out, (unsigned char*)out_u8, 3, plane, Hp, Wp, pad_top, pad_left, H, W, bgr ? 1 : 0};
    const bool vec = plane % 4 == 0 && atmvfi::aligned16(pred) && atmvfi::aligned16(pred_flip) && (!out || atmvfi::aligned16(out));
    const dim3 block(256);
    if (vec) hipLaunchKernelGGL((tta_merge_kernel<true, false>), dim3(capped_grid(plane / 4, 8192)), block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((tta_merge_kernel<false, false>), dim3(capped_grid(plane, 8192)), block, 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("tta_merge");
}

extern "C" int atmvfi_frame_rot180(const float* src, float* dst, int C, int Hp, int Wp, void* stream) {
    ATMVFI_REQUIRE(src && dst, ATMVFI_EINVAL, "frame_rot180: null pointer");
    ATMVFI_REQUIRE(src != dst, ATMVFI_EINVAL, "frame_rot180: in place is not supported");
    ATMVFI_REQUIRE(C > 0 && Hp > 0 && Wp > 0 && (long long)Hp * Wp < (1ll << 31) && (long long)C * Hp * Wp < (1ll << 40), ATMVFI_EINVAL,
                   "frame_rot180: bad shape [%d,%d,%d]", C, Hp, Wp);
    const long long plane = (long long)Hp * Wp;
    const MergeArgs a = {nullptr, src, dst, nullptr, C, plane, Hp, Wp, 0, 0, 0, 0, 0};
    const bool vec = plane % 4 == 0 && atmvfi::aligned16(src) && atmvfi::aligned16(dst);
    const dim3 block(256);
    if (vec) hipLaunchKernelGGL((tta_merge_kernel<true, true>), dim3(capped_grid(plane / 4 * C, 8192)), block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((tta_merge_kernel<false, true>), dim3(capped_grid(plane * C, 8192)), block, 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("frame_rot180");
}
