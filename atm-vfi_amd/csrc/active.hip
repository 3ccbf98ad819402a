// Active picture of letterboxed video in the N-x loop (include/atmvfi.h, atmvfi_frame_borders / atmvfi_frame_compose; ABI 0.21;
// atm-vfi_amd/active.py holds the policy and the host twins).  Nothing of the reference: its scripts only see full-picture clips.
//
// frame_borders: one resident uint8 [H,W,3] frame -> int32 out[H + W]:
//   luma        Y = (77 R + 150 G + 29 B + 128) >> 8            (the signature's own, scene.hip; R is byte 2 of a pixel when `bgr`)
//   out[y]      = max of Y over row y,      out[H + x] = max of Y over column x
// Integer work only: any reduction order gives the same bits, and the result equals the loop model (tests/cpu_active.py) exactly.
// Built as scene.hip is: bandwidth-bound (6.2 MB read at 1080p, 26.5 MB at 4K), two launches in one call, no global atomics, nothing
// to pre-zero, caller-provided workspace:
//   partial kernel: grid (column tiles of 1024 pixels, row chunks), 256 lanes.  A lane owns 4 horizontally adjacent pixels (12
//       contiguous bytes: three dwords on the aligned path) and walks down the rows of its chunk, 8 rows of loads in flight at a time.
//       Its four column maxima stay in registers for the whole chunk and leave as ONE dword (luma <= 255: a byte each).  The 8 row
//       maxima of a step are reduced over the wave by a butterfly that halves the number of values a lane carries while it still can
//       (4 + 2 + 1 exchanges, then 3 plain ones: 10 shuffles for 8 rows instead of 48); lane 8 r ends with row r and the wave writes
//       its 8 words.  No LDS, no barrier.  A maximum does not mind a row counted twice, so the rows past the chunk's end are the
//       chunk's last row again; lanes and pixels right of the frame carry 0, the identity of a maximum of lumas.
//   reduce kernel: a row takes the maximum over the 4 x tiles waves that saw it, a column over the chunks; 64 rows or 64 column
//       words per workgroup, its 16 waves each a slice of the partials, joined in LDS.
//
// frame_compose: dst uint8 [H,W,3] = the bytes of `border` outside the window (y0, x0, h, w) and the produced window inside -- from
//   src, fp32 planar [3,Hp,Wp] with the window at (pad_top, pad_left): frame_f32_to_u8's pixel (x * 255 in fp32, round half to even,
//   clamp, RGB -> BGR if `bgr`); or from win_u8, uint8 [h,w,3] already in output order.  A lane owns 4 horizontally adjacent pixels of
//   dst, grid-stride, 256 lanes.
//   aligned path: a group of four lies wholly inside or wholly outside the window (W, x0, w multiples of 4): 12-byte RGB groups of
//       border / win_u8 / dst as three dwords, 16-byte plane reads of src.
//   general path: any geometry and pointer alignment: bytes and scalars, the same arithmetic.
// Only the bar region of `border` is read, only the window of src / win_u8.
#include "common.h"

namespace {

constexpr int kRows = 8;                 // rows of loads in flight per lane
constexpr int kTilePixels = 1024;        // 256 lanes x 4 pixels
constexpr int kMaxRowsPerChunk = 256;
constexpr long long kMaxBlocks = 4096;

struct alignas(4) U32x3 {
    unsigned a, b, c;
};

struct BorderArgs {
    const unsigned char* src;
    long long pitch;        // 3 * W
    int H, W;
    int rows_per_chunk, groups;
    int w0, w2;             // luma weights of bytes 0 and 2 (77 / 29, swapped for BGR)
    int* rowp;              // [tiles * 4][H]: the row maxima each wave saw
    unsigned* colp;         // [chunks][groups]: four column maxima per word
};

struct BorderGeometry {
    int tiles, chunks, rows_per_chunk, groups;
    long long ints(int H) const { return 4ll * tiles * H + (long long)chunks * groups; }
};

// the launch geometry of a frame; shared by the workspace query and the launch
inline BorderGeometry geometry(int H, int W) {
    BorderGeometry g;
    g.tiles = (W + kTilePixels - 1) / kTilePixels;
    g.groups = (W + 3) / 4;
    long long rpc = kRows;
    while (rpc < kMaxRowsPerChunk && (long long)g.tiles * ((H + rpc - 1) / rpc) > kMaxBlocks) rpc += kRows;
    g.rows_per_chunk = (int)rpc;
    g.chunks = (int)((H + rpc - 1) / rpc);
    return g;
}

__device__ __forceinline__ int luma_of(const unsigned (&d)[3], int i, int w0, int w2) {
    const int b0 = (d[(3 * i) >> 2] >> (((3 * i) & 3) * 8)) & 0xff;
    const int b1 = (d[(3 * i + 1) >> 2] >> (((3 * i + 1) & 3) * 8)) & 0xff;
    const int b2 = (d[(3 * i + 2) >> 2] >> (((3 * i + 2) & 3) * 8)) & 0xff;
    return (w0 * b0 + 150 * b1 + w2 * b2 + 128) >> 8;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void frame_borders_partial_kernel(const BorderArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int ya = blockIdx.y * a.rows_per_chunk;
    const int yb = min(a.H, ya + a.rows_per_chunk);
    const int x = blockIdx.x * kTilePixels + tid * 4;         // column of the lane's first pixel
    const bool live = x < a.W;
    const int xl = ALIGNED ? x : min(x, a.W - 1);
    const unsigned char* base = a.src + (long long)(live ? xl : 0) * 3;
    int* const rows = a.rowp + (long long)(blockIdx.x * 4 + (tid >> 6)) * a.H;
    int col[4] = {0, 0, 0, 0};
    for (int yy = ya; yy < yb; yy += kRows) {
        int m[kRows];
        if (live) {
            unsigned d[kRows][3];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const unsigned char* p = base + (long long)min(yy + r, yb - 1) * a.pitch;        // clamped: always a row of the chunk
                if (ALIGNED) {
                    const U32x3 v = *reinterpret_cast<const U32x3*>(p);
                    d[r][0] = v.a; d[r][1] = v.b; d[r][2] = v.c;
                } else {
                    d[r][0] = d[r][1] = d[r][2] = 0u;
#pragma unroll
                    for (int k = 0; k < 12; ++k)
                        if (x + k / 3 < a.W) d[r][k >> 2] |= (unsigned)p[k] << ((k & 3) * 8);      // never a byte right of the frame
                }
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                m[r] = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (ALIGNED || x + i < a.W) {
                        const int y = luma_of(d[r], i, a.w0, a.w2);
                        m[r] = max(m[r], y);
                        col[i] = max(col[i], y);
                    }
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < kRows; ++r) m[r] = 0;
        }
        // 8 values over 64 lanes: bit 5 of the lane number chooses rows 0-3 / 4-7, bit 4 then a pair of those, bit 3 one row; a lane
        // sends the half it gives up and keeps the other.  After the three plain exchanges every lane holds the maximum of row lane >> 3
#pragma unroll
        for (int half = 4, bit = 32; half >= 1; half >>= 1, bit >>= 1) {
            const bool up = (lane & bit) != 0;
#pragma unroll
            for (int k = 0; k < half; ++k) {
                const int send = up ? m[k] : m[k + half], keep = up ? m[k + half] : m[k];
                m[k] = max(keep, __shfl_xor(send, bit));
            }
        }
        int v = m[0];
        v = max(v, __shfl_xor(v, 4));
        v = max(v, __shfl_xor(v, 2));
        v = max(v, __shfl_xor(v, 1));
        const int y = yy + (lane >> 3);
        if ((lane & 7) == 0 && y < yb) rows[y] = v;
    }
    if (live)
        a.colp[(long long)blockIdx.y * a.groups + (x >> 2)] =
            (unsigned)col[0] | ((unsigned)col[1] << 8) | ((unsigned)col[2] << 16) | ((unsigned)col[3] << 24);
}

// the maximum of each of the four bytes of two words
__device__ __forceinline__ unsigned max4(unsigned a, unsigned b) {
    unsigned r = 0u;
#pragma unroll
    for (int i = 0; i < 32; i += 8) r |= max((a >> i) & 0xffu, (b >> i) & 0xffu) << i;
    return r;
}

// A workgroup of 16 waves owns 64 items -- rows (a word per wave that saw the row, the maximum in byte 0) or column words (a word per
// chunk, four columns) -- lane = item, wave = a slice of the partials: the loads of a slice are independent and few (270 chunks at 4K
// are 17 per wave), where one lane per output word would walk them one latency after the other.  LDS joins the slices.
constexpr int kSlices = 16;
__global__ __launch_bounds__(64 * kSlices) void frame_borders_reduce_kernel(const unsigned* rowp, const unsigned* colp, int H, int W, int waves,
                                                                            int chunks, int groups, int row_blocks, int* out) {
    __shared__ unsigned red[kSlices][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const bool rows = (int)blockIdx.x < row_blocks;
    const int item = (rows ? blockIdx.x : blockIdx.x - row_blocks) * 64 + lane;
    const int items = rows ? H : groups, count = rows ? waves : chunks;
    const unsigned* base = (rows ? rowp : colp) + min(item, items - 1);
    unsigned acc = 0u;                                        // lumas are >= 0: the identity
#pragma unroll 4
    for (int k = slice; k < count; k += kSlices) acc = max4(acc, base[(long long)k * items]);
    red[slice][lane] = acc;
    __syncthreads();
    if (slice != 0 || item >= items) return;
#pragma unroll
    for (int s = 1; s < kSlices; ++s) acc = max4(acc, red[s][lane]);
    if (rows) {
        out[item] = (int)(acc & 0xffu);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * item + i < W) out[H + 4 * item + i] = (int)((acc >> (8 * i)) & 0xffu);
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int check_frame(const char* what, int H, int W) {
    ATMVFI_REQUIRE(H >= 16 && W >= 16, ATMVFI_EINVAL, "%s: the frame must be at least 16 x 16 (got %d x %d)", what, H, W);
    ATMVFI_REQUIRE((long long)H * W <= 0x7fffffffll, ATMVFI_EINVAL, "%s: a %d x %d frame is too large (H * W must fit int32)", what, H, W);
    ATMVFI_REQUIRE(geometry(H, W).chunks <= 65535, ATMVFI_EINVAL, "%s: a %d x %d frame is too large (%d row chunks, at most 65535)", what, H, W,
                   geometry(H, W).chunks);
    return ATMVFI_OK;
}

// ------------------------------------------------------------------------------------------------ compose
struct ComposeArgs {
    unsigned char* dst;
    const unsigned char* border;
    const float* src;
    const unsigned char* win;
    int H, W, y0, x0, h, w;
    int Hp, Wp, pad_top, pad_left;
    int groups;             // ceil(W / 4)
};

__device__ __forceinline__ int to_u8(float v) {
    const int q = __float2int_rn(v * 255.0f);                 // rint: half to even, as np.round (frame_f32_to_u8)
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void frame_compose_kernel(const ComposeArgs a, const int bgr) {
    const long long plane = (long long)a.Hp * a.Wp;
    const int total = a.H * a.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int y = idx / a.groups, x = (idx - y * a.groups) * 4;
        const int wy = y - a.y0, wx = x - a.x0;               // window coordinates of the group's first pixel
        const bool row_in = wy >= 0 && wy < a.h;
        const long long at = ((long long)y * a.W + x) * 3;
        if (ALIGNED) {
            U32x3 o;
            if (!(row_in && wx >= 0 && wx < a.w)) {
                o = *reinterpret_cast<const U32x3*>(a.border + at);
            } else if (a.win) {
                o = *reinterpret_cast<const U32x3*>(a.win + ((long long)wy * a.w + wx) * 3);
            } else {
                const float* p = a.src + (long long)(wy + a.pad_top) * a.Wp + (wx + a.pad_left);
                const f32x4 c0 = *reinterpret_cast<const f32x4*>(p + (bgr ? 2 * plane : 0));
                const f32x4 c1 = *reinterpret_cast<const f32x4*>(p + plane);
                const f32x4 c2 = *reinterpret_cast<const f32x4*>(p + (bgr ? 0 : 2 * plane));
                unsigned d[3] = {0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int q[3] = {to_u8(c0[i]), to_u8(c1[i]), to_u8(c2[i])};
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[(3 * i + c) >> 2] |= (unsigned)q[c] << (((3 * i + c) & 3) * 8);
                }
                o = U32x3{d[0], d[1], d[2]};
            }
            *reinterpret_cast<U32x3*>(a.dst + at) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.W) break;
                unsigned char* o = a.dst + at + 3 * i;
                if (!(row_in && wx + i >= 0 && wx + i < a.w)) {
                    const unsigned char* p = a.border + at + 3 * i;
                    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
                } else if (a.win) {
                    const unsigned char* p = a.win + ((long long)wy * a.w + wx + i) * 3;
                    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
                } else {
                    const float* p = a.src + (long long)(wy + a.pad_top) * a.Wp + (wx + i + a.pad_left);
                    const int q0 = to_u8(p[0]), q1 = to_u8(p[plane]), q2 = to_u8(p[2 * plane]);
                    o[0] = (unsigned char)(bgr ? q2 : q0);
                    o[1] = (unsigned char)q1;
                    o[2] = (unsigned char)(bgr ? q0 : q2);
                }
            }
        }
    }
}

}  // namespace

extern "C" int64_t atmvfi_frame_borders_workspace_ints(int H, int W) {
    if (check_frame("frame_borders_workspace_ints", H, W) != ATMVFI_OK) return -1;
    return geometry(H, W).ints(H);
}

extern "C" int atmvfi_frame_borders(const void* src, int H, int W, int bgr, int32_t* out, int32_t* workspace, int64_t workspace_ints,
                                    void* stream) {
    ATMVFI_REQUIRE(src && out && workspace, ATMVFI_EINVAL, "frame_borders: null pointer (src %p, out %p, workspace %p)", src, (void*)out,
                   (void*)workspace);
    if (const int rc = check_frame("frame_borders", H, W)) return rc;
    ATMVFI_REQUIRE(aligned4(out) && aligned4(workspace), ATMVFI_EINVAL, "frame_borders: out and workspace must be 4-byte aligned");
    const BorderGeometry g = geometry(H, W);
    ATMVFI_REQUIRE(workspace_ints >= g.ints(H), ATMVFI_EINVAL,
                   "frame_borders: workspace of %lld ints, %lld needed (atmvfi_frame_borders_workspace_ints)", (long long)workspace_ints,
                   g.ints(H));
    // aligned path: every lane's 12 bytes are three dwords and lie inside the frame (W % 4 == 0: no group reads past a row's end)
    const bool al = aligned4(src) && W % 4 == 0;
    int* const rowp = workspace;
    unsigned* const colp = reinterpret_cast<unsigned*>(workspace + 4ll * g.tiles * H);
    const BorderArgs a = {(const unsigned char*)src, 3ll * W, H, W, g.rows_per_chunk, g.groups, bgr ? 29 : 77, bgr ? 77 : 29, rowp, colp};
    const dim3 grid((unsigned)g.tiles, (unsigned)g.chunks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (al) hipLaunchKernelGGL((frame_borders_partial_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((frame_borders_partial_kernel<false>), grid, block, 0, st, a);
    if (const int rc = atmvfi::check_launch("frame_borders (partials)")) return rc;
    const int row_blocks = (H + 63) / 64, col_blocks = (g.groups + 63) / 64;
    hipLaunchKernelGGL(frame_borders_reduce_kernel, dim3((unsigned)(row_blocks + col_blocks)), dim3(64 * kSlices), 0, st, (const unsigned*)rowp,
                       (const unsigned*)colp, H, W, 4 * g.tiles, g.chunks, g.groups, row_blocks, out);
    return atmvfi::check_launch("frame_borders (reduce)");
}

extern "C" int atmvfi_frame_compose(void* dst, const void* border, int H, int W, int y0, int x0, int h, int w, const float* src, int Hp, int Wp,
                                    int pad_top, int pad_left, const void* win_u8, int bgr, void* stream) {
    ATMVFI_REQUIRE(dst && border, ATMVFI_EINVAL, "frame_compose: null pointer (dst %p, border %p)", dst, border);
    ATMVFI_REQUIRE((src != nullptr) != (win_u8 != nullptr), ATMVFI_EINVAL, "frame_compose: give exactly one of src and win_u8");
    ATMVFI_REQUIRE(H > 0 && W > 0 && y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && (long long)y0 + h <= H && (long long)x0 + w <= W, ATMVFI_EINVAL,
                   "frame_compose: window outside the frame (%d x %d at (%d, %d) of a %d x %d frame)", h, w, y0, x0, H, W);
    const int groups = (int)(((long long)W + 3) / 4);
    ATMVFI_REQUIRE((long long)H * groups < (1ll << 30), ATMVFI_EINVAL, "frame_compose: a frame of %d x %d is too large", H, W);
    const long long bytes = 3ll * H * W;
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst), b = reinterpret_cast<uintptr_t>(border);
    ATMVFI_REQUIRE(d + (uintptr_t)bytes <= b || b + (uintptr_t)bytes <= d, ATMVFI_EINVAL,
                   "frame_compose: dst must not alias border (dst %p, border %p, %lld bytes each)", dst, border, bytes);
    if (src) {
        ATMVFI_REQUIRE(Hp > 0 && Wp > 0 && pad_top >= 0 && pad_left >= 0 && (long long)h + pad_top <= Hp && (long long)w + pad_left <= Wp &&
                           (long long)Hp * Wp < (1ll << 31),
                       ATMVFI_EINVAL, "frame_compose: bad geometry (Hp %d Wp %d, window %d x %d, pad %d %d)", Hp, Wp, h, w, pad_top, pad_left);
    }
    // aligned path: a group of four is wholly inside or outside the window, every RGB group three dwords, every plane read 16 bytes
    const bool al = aligned4(dst) && aligned4(border) && W % 4 == 0 && x0 % 4 == 0 && w % 4 == 0 &&
                    (src ? (atmvfi::aligned16(src) && Wp % 4 == 0 && pad_left % 4 == 0) : aligned4(win_u8));
    const ComposeArgs a = {(unsigned char*)dst, (const unsigned char*)border, src, (const unsigned char*)win_u8, H, W, y0, x0, h, w,
                           Hp, Wp, pad_top, pad_left, groups};
    const long long blocks = ((long long)H * groups + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks)), block(256);
    if (al) hipLaunchKernelGGL((frame_compose_kernel<true>), grid, block, 0, (hipStream_t)stream, a, bgr ? 1 : 0);
    else hipLaunchKernelGGL((frame_compose_kernel<false>), grid, block, 0, (hipStream_t)stream, a, bgr ? 1 : 0);
    return atmvfi::check_launch("frame_compose");
}
