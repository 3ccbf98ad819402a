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
//
// The same on YUV streams (atmvfi_yuv_borders / atmvfi_yuv_compose; ABI 0.22; active.py: bar_code, yuv_borders_numpy, yuv_compose_numpy;
// models tests/cpu_yuv_active.py):
// yuv_borders: the luma plane of a resident frame or surface -> int32 out[H + W], the largest sample value per row and per column.
//   The partial kernel is frame_borders' with the lane's four samples as ONE dword (8 bit) or 8 bytes (10 bit) and no colour
//   arithmetic; the wave's row butterfly and the reduce kernel are shared.  Raw stored samples are compared (a maximum commutes
//   with the msb shift), the reduce kernel shifts once.  Column maxima leave as a byte each (8 bit) or a half-word each (10 bit).
// yuv_compose: dst, one tight frame = the samples of `border` (a surface of any pitch) outside the window, the window's encode inside.
//   bars:   at most four rectangles of bytes per plane (above, below, left and right of the window; an interleaved chroma plane is one
//           plane of pairs), blockIdx.y the rectangle, a lane 16 bytes of a line: dwords where the rectangle's origins and pitches are
//           multiples of 4 bytes, bytes else and in a line's tail.  No sample of the window is touched.  The stored samples move as
//           they are; of an msb word the value's ten bits (the low six leave as zero: what yuv.repack and the encode write).
//   window: the encode kernel of yuv_encode.hip itself, launched with the window's origin in the frame (atmvfi::yuv_encode_window):
//           the arithmetic exists once.  The window rule makes every chroma sample the window's or the bars'.
#include "yuv_common.h"

namespace {

constexpr int kRows = 8;                 // rows of loads in flight per lane
constexpr int kTilePixels = 1024;        // 256 lanes x 4 pixels
constexpr int kMaxRowsPerChunk = 256;
constexpr long long kMaxBlocks = 4096;

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

// 8 values over 64 lanes: bit 5 of the lane number chooses rows 0-3 / 4-7, bit 4 then a pair of those, bit 3 one row; a lane sends the
// half it gives up and keeps the other.  After the three plain exchanges every lane holds the maximum of row lane >> 3
__device__ __forceinline__ int wave_rows(int (&m)[kRows], int lane) {
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
    return v;
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
        const int v = wave_rows(m, lane);
        const int y = yy + (lane >> 3);
        if ((lane & 7) == 0 && y < yb) rows[y] = v;
    }
    if (live)
        a.colp[(long long)blockIdx.y * a.groups + (x >> 2)] =
            (unsigned)col[0] | ((unsigned)col[1] << 8) | ((unsigned)col[2] << 16) | ((unsigned)col[3] << 24);
}

// the maximum of each of the PER fields (four bytes, or two half-words) of two words
template <int PER>
__device__ __forceinline__ unsigned maxp(unsigned a, unsigned b) {
    constexpr int BITS = 32 / PER;
    constexpr unsigned MASK = (1u << BITS) - 1u;
    unsigned r = 0u;
#pragma unroll
    for (int i = 0; i < 32; i += BITS) r |= max((a >> i) & MASK, (b >> i) & MASK) << i;
    return r;
}

// A workgroup of 16 waves owns 64 items -- rows (a word per wave that saw the row, the maximum in field 0) or column words (a word per
// chunk, PER columns: four bytes, or two half-words for 10-bit samples) -- lane = item, wave = a slice of the partials: the loads of a
// slice are independent and few (270 chunks at 4K are 17 per wave), where one lane per output word would walk them one latency after
// the other.  LDS joins the slices.  shift: what takes a stored sample to its value (6 for msb samples, else 0).
constexpr int kSlices = 16;
template <int PER>
__global__ __launch_bounds__(64 * kSlices) void frame_borders_reduce_kernel(const unsigned* rowp, const unsigned* colp, int H, int W, int waves,
                                                                            int chunks, int groups, int row_blocks, int shift, int* out) {
    constexpr int BITS = 32 / PER;
    constexpr unsigned MASK = (1u << BITS) - 1u;
    __shared__ unsigned red[kSlices][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const bool rows = (int)blockIdx.x < row_blocks;
    const int item = (rows ? blockIdx.x : blockIdx.x - row_blocks) * 64 + lane;
    const int items = rows ? H : groups, count = rows ? waves : chunks;
    const unsigned* base = (rows ? rowp : colp) + min(item, items - 1);
    unsigned acc = 0u;                                        // samples are >= 0: the identity
#pragma unroll 4
    for (int k = slice; k < count; k += kSlices) acc = maxp<PER>(acc, base[(long long)k * items]);
    red[slice][lane] = acc;
    __syncthreads();
    if (slice != 0 || item >= items) return;
#pragma unroll
    for (int s = 1; s < kSlices; ++s) acc = maxp<PER>(acc, red[s][lane]);
    if (rows) {
        out[item] = (int)((acc & MASK) >> shift);
    } else {
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (PER * item + i < W) out[H + PER * item + i] = (int)(((acc >> (BITS * i)) & MASK) >> shift);
    }
}

// ------------------------------------------------------------------------------------------------ the luma plane of a YUV frame
struct YBorderArgs {
    const unsigned char* src;
    long long pitch;        // bytes
    int H, W;
    int rows_per_chunk, groups;
    int* rowp;              // [tiles * 4][H]
    unsigned* colp;         // depth 8: [chunks][groups], four columns per word; depth 10: [chunks][2 groups], two columns per word
};

template <int DEPTH, bool ALIGNED>
__global__ __launch_bounds__(256) void yuv_borders_partial_kernel(const YBorderArgs a) {
    constexpr int B = DEPTH == 8 ? 1 : 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ya = blockIdx.y * a.rows_per_chunk;
    const int yb = min(a.H, ya + a.rows_per_chunk);
    const int x = blockIdx.x * kTilePixels + tid * 4;         // column of the lane's first sample
    const bool live = x < a.W;
    const unsigned char* base = a.src + (long long)(live ? x : 0) * B;
    int* const rows = a.rowp + (long long)(blockIdx.x * 4 + (tid >> 6)) * a.H;
    int col[4] = {0, 0, 0, 0};
    for (int yy = ya; yy < yb; yy += kRows) {
        int m[kRows];
        if (live) {
            int s[kRows][4];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const unsigned char* p = base + (long long)min(yy + r, yb - 1) * a.pitch;        // clamped: always a row of the chunk
                if (ALIGNED) {
                    if (DEPTH == 8) {
                        const unsigned d = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
                        for (int i = 0; i < 4; ++i) s[r][i] = (int)((d >> (8 * i)) & 0xffu);
                    } else {
                        const U32x2 d = *reinterpret_cast<const U32x2*>(p);
                        s[r][0] = (int)(d.a & 0xffffu);
                        s[r][1] = (int)(d.a >> 16);
                        s[r][2] = (int)(d.b & 0xffffu);
                        s[r][3] = (int)(d.b >> 16);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        s[r][i] = 0;                           // never a byte right of the row's samples
                        if (x + i < a.W) s[r][i] = DEPTH == 8 ? (int)p[i] : (int)((unsigned)p[2 * i] | ((unsigned)p[2 * i + 1] << 8));
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                m[r] = max(max(s[r][0], s[r][1]), max(s[r][2], s[r][3]));
#pragma unroll
                for (int i = 0; i < 4; ++i) col[i] = max(col[i], s[r][i]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < kRows; ++r) m[r] = 0;
        }
        const int v = wave_rows(m, lane);
        const int y = yy + (lane >> 3);
        if ((lane & 7) == 0 && y < yb) rows[y] = v;
    }
    if (!live) return;
    if (DEPTH == 8) {
        a.colp[(long long)blockIdx.y * a.groups + (x >> 2)] =
            (unsigned)col[0] | ((unsigned)col[1] << 8) | ((unsigned)col[2] << 16) | ((unsigned)col[3] << 24);
    } else {
        *reinterpret_cast<U32x2*>(a.colp + ((long long)blockIdx.y * a.groups + (x >> 2)) * 2) =
            U32x2{(unsigned)col[0] | ((unsigned)col[1] << 16), (unsigned)col[2] | ((unsigned)col[3] << 16)};
    }
}

// ------------------------------------------------------------------------------------------------ the bars of a YUV frame
struct alignas(4) U32x4 {
    unsigned a, b, c, d;
};

// `lines` lines of `bytes` bytes from border + src to dst + dst_off, a lane 16 bytes of a line
struct BarRect {
    long long src, dst, src_pitch, dst_pitch;
    int lines, groups, bytes, aligned;
};
constexpr int kMaxRects = 12;                // four around the window per plane
struct BarArgs {
    unsigned char* dst;
    const unsigned char* border;
    unsigned mask;          // 0xffc0ffc0 for msb samples (the value's ten bits move, as yuv.repack writes them), else all ones
    BarRect r[kMaxRects];
};

__global__ __launch_bounds__(256) void yuv_bars_kernel(const BarArgs a) {
    const BarRect& r = a.r[blockIdx.y];       // (uniform: scalar loads of the kernel's arguments)
    const int total = r.lines * r.groups;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int line = idx / r.groups, at = (idx - line * r.groups) * 16;
        const unsigned char* s = a.border + r.src + (long long)line * r.src_pitch + at;
        unsigned char* d = a.dst + r.dst + (long long)line * r.dst_pitch + at;
        const int n = min(16, r.bytes - at);
        // (a sample of two bytes begins on an even byte of its line, and `at` is even: byte k is a low byte iff k is even)
        if (r.aligned && n == 16) {
            const U32x4 v = *reinterpret_cast<const U32x4*>(s);
            *reinterpret_cast<U32x4*>(d) = U32x4{v.a & a.mask, v.b & a.mask, v.c & a.mask, v.d & a.mask};
        } else if (r.aligned) {                // a line's tail: dwords, then bytes
            int k = 0;
            for (; k + 4 <= n; k += 4) *reinterpret_cast<unsigned*>(d + k) = *reinterpret_cast<const unsigned*>(s + k) & a.mask;
            for (; k < n; ++k) d[k] = (unsigned char)(s[k] & (a.mask >> (8 * (k & 1))));
        } else {
            for (int k = 0; k < n; ++k) d[k] = (unsigned char)(s[k] & (a.mask >> (8 * (k & 1))));
        }
    }
}

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
    hipLaunchKernelGGL(frame_borders_reduce_kernel<4>, dim3((unsigned)(row_blocks + col_blocks)), dim3(64 * kSlices), 0, st, (const unsigned*)rowp,
                       (const unsigned*)colp, H, W, 4 * g.tiles, g.chunks, g.groups, row_blocks, 0, out);
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

// ------------------------------------------------------------------------------------------------ YUV (ABI 0.22)
// (the workspace of the 10-bit partials, two column words per group: what either depth fits into)
extern "C" int64_t atmvfi_yuv_borders_workspace_ints(int H, int W) {
    if (check_frame("yuv_borders_workspace_ints", H, W) != ATMVFI_OK) return -1;
    const BorderGeometry g = geometry(H, W);
    return g.ints(H) + (long long)g.chunks * g.groups;
}

extern "C" int atmvfi_yuv_borders(const atmvfi_yuv_desc* desc, const void* yuv, int32_t* out, int32_t* workspace, int64_t workspace_ints,
                                  void* stream) {
    ATMVFI_REQUIRE(desc, ATMVFI_EINVAL, "yuv_borders: null descriptor");
    const int H = desc->H, W = desc->W, depth = desc->depth, msb = desc->msb;
    long long pitch = desc->pitch;
    ATMVFI_REQUIRE(yuv && out && workspace, ATMVFI_EINVAL, "yuv_borders: null pointer (yuv %p, out %p, workspace %p)", yuv, (void*)out,
                   (void*)workspace);
    if (const int rc = check_frame("yuv_borders", H, W)) return rc;
    ATMVFI_REQUIRE(depth == 8 || depth == 10, ATMVFI_EINVAL, "yuv_borders: depth must be 8 or 10 (got %d)", depth);
    ATMVFI_REQUIRE(msb == 0 || (msb == 1 && depth == 10), ATMVFI_EINVAL, "yuv_borders: msb must be 0 or 1 and needs depth 10 (got msb %d, depth %d)",
                   msb, depth);
    const long long b = depth == 10 ? 2 : 1;
    if (pitch == 0) pitch = W * b;
    ATMVFI_REQUIRE(pitch % b == 0 && pitch >= W * b, ATMVFI_EINVAL,
                   "yuv_borders: pitch %lld must be a multiple of the sample size %lld and at least a luma row's %lld bytes", pitch, b, W * b);
    ATMVFI_REQUIRE(aligned4(out) && aligned4(workspace), ATMVFI_EINVAL, "yuv_borders: out and workspace must be 4-byte aligned");
    const BorderGeometry g = geometry(H, W);
    const long long need = g.ints(H) + (long long)g.chunks * g.groups;
    ATMVFI_REQUIRE(workspace_ints >= need, ATMVFI_EINVAL, "yuv_borders: workspace of %lld ints, %lld needed (atmvfi_yuv_borders_workspace_ints)",
                   (long long)workspace_ints, need);
    // vector path: a lane's four samples are one dword / 8 bytes of their row and lie inside it
    const bool al = aligned4(yuv) && pitch % 4 == 0 && W % 4 == 0;
    int* const rowp = workspace;
    unsigned* const colp = reinterpret_cast<unsigned*>(workspace + 4ll * g.tiles * H);
    const YBorderArgs a = {(const unsigned char*)yuv, pitch, H, W, g.rows_per_chunk, g.groups, rowp, colp};
    const dim3 grid((unsigned)g.tiles, (unsigned)g.chunks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    dispatch([&](auto D10, auto AL) {
        hipLaunchKernelGGL((yuv_borders_partial_kernel<D10() ? 10 : 8, AL()>), grid, block, 0, st, a);
    }, depth == 10, al);
    if (const int rc = atmvfi::check_launch("yuv_borders (partials)")) return rc;
    const int words = depth == 10 ? 2 * g.groups : g.groups;       // column words per chunk
    const int row_blocks = (H + 63) / 64, col_blocks = (words + 63) / 64;
    const dim3 rgrid((unsigned)(row_blocks + col_blocks)), rblock(64 * kSlices);
    if (depth == 10)
        hipLaunchKernelGGL(frame_borders_reduce_kernel<2>, rgrid, rblock, 0, st, (const unsigned*)rowp, (const unsigned*)colp, H, W, 4 * g.tiles,
                           g.chunks, words, row_blocks, msb ? 6 : 0, out);
    else
        hipLaunchKernelGGL(frame_borders_reduce_kernel<4>, rgrid, rblock, 0, st, (const unsigned*)rowp, (const unsigned*)colp, H, W, 4 * g.tiles,
                           g.chunks, words, row_blocks, 0, out);
    return atmvfi::check_launch("yuv_borders (reduce)");
}

extern "C" int atmvfi_yuv_compose(const atmvfi_yuv_desc* border_desc, void* dst, const void* border, int y0, int x0, int h, int w,
                                  const float* src, int Hp, int Wp, int pad_top, int pad_left, const void* src_u8, void* stream) {
    const char* me = "yuv_compose";
    ATMVFI_REQUIRE(border_desc, ATMVFI_EINVAL, "%s: null descriptor", me);
    const atmvfi_yuv_desc& bd = *border_desc;
    const int H = bd.H, W = bd.W, depth = bd.depth, subsampling = bd.subsampling, chroma = bd.chroma, msb = bd.msb;
    ATMVFI_REQUIRE(dst && border, ATMVFI_EINVAL, "%s: null pointer (dst %p, border %p)", me, dst, border);
    ATMVFI_REQUIRE((src != nullptr) != (src_u8 != nullptr), ATMVFI_EINVAL, "%s: give exactly one of src and src_u8", me);
    if (const int rc = check_format(me, bd)) return rc;
    if (const int rc = check_depth(me, bd)) return rc;
    if (const int rc = check_sub(me, bd)) return rc;
    Layout bl;
    if (const int rc = check_surface(me, bd, &bl)) return rc;
    ATMVFI_REQUIRE(y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && (long long)y0 + h <= H && (long long)x0 + w <= W, ATMVFI_EINVAL,
                   "%s: window outside the frame (%d x %d at (%d, %d) of a %d x %d frame)", me, h, w, y0, x0, H, W);
    const int sy = subsampling == 0 ? 2 : 1, sx = subsampling == 2 ? 1 : 2;
    ATMVFI_REQUIRE(y0 % sy == 0 && x0 % sx == 0 && ((y0 + h) % sy == 0 || y0 + h == H) && ((x0 + w) % sx == 0 || x0 + w == W), ATMVFI_EINVAL,
                   "%s: the window %d x %d at (%d, %d) must begin and end on multiples of the subsampling step (%d, %d) or at the frame's edge", me,
                   h, w, y0, x0, sy, sx);
    ATMVFI_REQUIRE((long long)H * W < (1ll << 30), ATMVFI_EINVAL, "%s: a frame of %d x %d is too large", me, H, W);
    const long long b = depth == 10 ? 2 : 1;
    const int ch = chroma_rows(H, subsampling), cw = chroma_cols(W, subsampling);
    const Layout tl = tight_layout(H, W, chroma, subsampling);
    const long long crow = (long long)(chroma ? 2 * cw : cw) * b, planes = chroma ? 1 : 2;
    const long long dst_bytes = ((long long)H * W + 2ll * ch * cw) * b;
    const long long border_bytes = (bl.uoff + (long long)bl.cs * (planes * ch - 1)) * b + crow;
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst), bo = reinterpret_cast<uintptr_t>(border);
    ATMVFI_REQUIRE(d + (uintptr_t)dst_bytes <= bo || bo + (uintptr_t)border_bytes <= d, ATMVFI_EINVAL,
                   "%s: dst must not overlap border (dst %p of %lld bytes, border %p of %lld bytes)", me, dst, dst_bytes, border, border_bytes);
    // the bars: per plane the lines above and below the window and, beside it, the bytes left and right of it
    BarArgs a = {(unsigned char*)dst, (const unsigned char*)border, msb ? 0xffc0ffc0u : 0xffffffffu};
    int rects = 0;
    long long most = 0;
    const bool base_al = aligned4(dst) && aligned4(border);
    auto rect = [&](long long s, long long sp, long long dd, long long dp, long long line0, long long lines, long long b0, long long b1) {
        if (lines <= 0 || b1 <= b0) return;
        BarRect& r = a.r[rects++];
        r = BarRect{s + line0 * sp + b0, dd + line0 * dp + b0, sp, dp, (int)lines, (int)((b1 - b0 + 15) / 16), (int)(b1 - b0), 0};
        r.aligned = base_al && r.src % 4 == 0 && r.dst % 4 == 0 && sp % 4 == 0 && dp % 4 == 0;
        most = most > lines * r.groups ? most : lines * r.groups;
    };
    auto plane = [&](long long s, long long sp, long long dd, long long dp, long long lines, long long bytes, long long l0, long long l1, long long b0,
                     long long b1) {
        rect(s, sp, dd, dp, 0, l0, 0, bytes);
        rect(s, sp, dd, dp, l1, lines - l1, 0, bytes);
        rect(s, sp, dd, dp, l0, l1 - l0, 0, b0);
        rect(s, sp, dd, dp, l0, l1 - l0, b1, bytes);
    };
    const long long cy0 = y0 / sy, cy1 = ((long long)y0 + h + sy - 1) / sy, cx0 = x0 / sx, cx1 = ((long long)x0 + w + sx - 1) / sx;
    plane(0, bl.ys * b, 0, tl.ys * b, H, W * b, y0, y0 + h, x0 * b, ((long long)x0 + w) * b);
    const long long e = chroma ? 2 : 1;        // samples per chroma column of a plane's line
    for (int p = 0; p < planes; ++p)
        plane((bl.uoff + (long long)p * ch * bl.cs) * b, bl.cs * b, (tl.uoff + (long long)p * ch * tl.cs) * b, tl.cs * b, ch, crow, cy0, cy1, cx0 * e * b,
              cx1 * e * b);
    // the window: every check of the encode, then its kernel at the window's origin
    if (const int rc = atmvfi::yuv_encode_window(me, bd, dst, y0, x0, h, w, src_u8, src, Hp, Wp, pad_top, pad_left, stream)) return rc;
    if (rects == 0) return ATMVFI_OK;           // the window is the frame
    const long long blocks = (most + 255) / 256;
    hipLaunchKernelGGL(yuv_bars_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)rects), dim3(256), 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("yuv_compose (bars)");
}
