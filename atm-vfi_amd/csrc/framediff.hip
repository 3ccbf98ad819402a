// Frame difference for duplicate-frame detection in the retimed video loop (include/atmvfi.h, atmvfi_frame_difference;
// atm-vfi_amd/retime.py): two resident uint8 [H,W,3] frames and a window (y0, x0, h, w) -> int32 out[258]:
//   luma        Y = (77 R + 150 G + 29 B + 128) >> 8            (the signature's own, scene.hip; R is byte 2 of a pixel when `bgr`)
//   out[16 i + j] = sum of |Ya - Yb| over rows [i h / 16, (i + 1) h / 16) x columns [j w / 16, (j + 1) w / 16)    (the signature's cells)
//   out[256]      = max |Ya - Yb| over the window
//   out[257]      = number of window pixels with Ya != Yb
// Integer work only: any reduction order gives the same bits, and the result equals the loop model (tests/cpu_framediff.py) exactly.
//
// Built as scene.hip is: bandwidth-bound (12.4 MB read at 1080p, 53 MB at 4K), two launches in one call, no global atomics, nothing to
// pre-zero, caller-provided workspace:
//   partial kernel: grid (column tiles of 1024 pixels, row chunks, 16 cell rows), 256 lanes.  A lane owns 4 horizontally adjacent
//       pixels of BOTH frames (12 contiguous bytes each: three dwords on the aligned path) and walks down the rows of its chunk, 4 rows
//       of loads of each frame in flight at a time (24 dwords, what the signature keeps in flight for its one frame).  The lane's pixel
//       columns, and with them its cell columns, are fixed: four SAD sums, the peak and the count stay in registers for the whole chunk.
//       At the end the sums are reduced per wave by a segmented shuffle scan (the cell column is monotone in the lane number), segment
//       heads add into 16 LDS words; peak and count are reduced by butterflies, one LDS word per wave.  The workgroup writes its 18
//       partial words to the caller's workspace.
//   reduce kernel: one wave per output word (258 waves) sums (word 256: maximises) the partials that belong to it.
#include "common.h"

namespace {

constexpr int kRows = 4;                 // rows of loads in flight per lane and frame
constexpr int kPartial = 18;             // words per workgroup: 16 cell-column sums of its cell row, the peak, the count
constexpr int kOutWords = 258;
constexpr int kTilePixels = 1024;        // 256 lanes x 4 pixels
constexpr long long kMaxBlocks = 4096;

struct alignas(4) U32x3 {
    unsigned a, b, c;
};

struct DiffArgs {
    const unsigned char* a;
    const unsigned char* b;
    long long pitch;        // 3 * W
    int y0, x0, h, w;
    int rows_per_chunk;
    int w0, w2;             // luma weights of bytes 0 and 2 (77 / 29, swapped for BGR)
    int* partial;
};

struct DiffGeometry {
    int tiles, chunks, rows_per_chunk;
    long long blocks() const { return 16ll * tiles * chunks; }
};

// the launch geometry of a window; shared by the workspace query and the launch
inline DiffGeometry geometry(int h, int w) {
    DiffGeometry g;
    g.tiles = (w + kTilePixels - 1) / kTilePixels;
    const int band = (h + 15) / 16;                          // the tallest cell row
    long long rpc = 2 * kRows;
    while (rpc < band && 16ll * g.tiles * ((band + rpc - 1) / rpc) > kMaxBlocks) rpc += 2 * kRows;
    g.rows_per_chunk = (int)rpc;
    g.chunks = (int)((band + rpc - 1) / rpc);
    return g;
}

template <bool ALIGNED>
__device__ __forceinline__ void load12(const unsigned char* p, int x, int w, unsigned (&d)[3]) {
    if (ALIGNED) {
        const U32x3 v = *reinterpret_cast<const U32x3*>(p);
        d[0] = v.a; d[1] = v.b; d[2] = v.c;
    } else {
        d[0] = d[1] = d[2] = 0u;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (x + k / 3 < w) d[k >> 2] |= (unsigned)p[k] << ((k & 3) * 8);      // never a byte of a pixel outside the window
    }
}

__device__ __forceinline__ int luma_of(const unsigned (&d)[3], int i, int w0, int w2) {
    const int b0 = (d[(3 * i) >> 2] >> (((3 * i) & 3) * 8)) & 0xff;
    const int b1 = (d[(3 * i + 1) >> 2] >> (((3 * i + 1) & 3) * 8)) & 0xff;
    const int b2 = (d[(3 * i + 2) >> 2] >> (((3 * i + 2) & 3) * 8)) & 0xff;
    return (w0 * b0 + 150 * b1 + w2 * b2 + 128) >> 8;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void frame_difference_partial_kernel(const DiffArgs a) {
    __shared__ int cells[16];
    __shared__ int wave_peak[4], wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 16) cells[tid] = 0;
    __syncthreads();

    const int band = blockIdx.z;
    const int r0 = (int)((long long)band * a.h / 16), r1 = (int)((long long)(band + 1) * a.h / 16);
    const int ya = r0 + blockIdx.y * a.rows_per_chunk;
    const int yb = min(r1, ya + a.rows_per_chunk);
    const int x = blockIdx.x * kTilePixels + tid * 4;         // window column of the lane's first pixel
    int sad[4] = {0, 0, 0, 0};
    int peak = 0, count = 0;
    if (x < a.w) {
        const int xl = ALIGNED ? x : min(x, a.w - 1);
        const long long off = (long long)a.y0 * a.pitch + (long long)(a.x0 + xl) * 3;
        const unsigned char* base_a = a.a + off;
        const unsigned char* base_b = a.b + off;
        for (int yy = ya; yy < yb; yy += kRows) {
            unsigned da[kRows][3], db[kRows][3];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const long long row = (long long)min(yy + r, yb - 1) * a.pitch;                    // clamped: always a row of the chunk
                load12<ALIGNED>(base_a + row, x, a.w, da[r]);
                load12<ALIGNED>(base_b + row, x, a.w, db[r]);
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                if (yy + r < yb) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (x + i < a.w) {
                            const int d = abs(luma_of(da[r], i, a.w0, a.w2) - luma_of(db[r], i, a.w0, a.w2));
                            sad[i] += d;
                            peak = max(peak, d);
                            count += d != 0;
                        }
                    }
                }
            }
        }
    }
    // cell column of window column c: the largest j with j * w / 16 <= c, i.e. (16 c + 15) / w; monotone in the lane number, so the
    // lanes of one cell are a contiguous run of the wave: a segmented shuffle scan leaves each run's total in its first lane
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = min(x + i, a.w - 1);
        const int j = (int)((16ll * c + 15) / a.w);
        int s = sad[i];
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int os = __shfl_down(s, dlt), oj = __shfl_down(j, dlt);
            if (lane + dlt < 64 && oj == j) s += os;
        }
        const int pj = __shfl_up(j, 1);
        if ((lane == 0 || pj != j) && s != 0) atomicAdd(&cells[j], s);       // LDS
    }
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) {
        peak = max(peak, __shfl_xor(peak, dlt));
        count += __shfl_xor(count, dlt);
    }
    if (lane == 0) {
        wave_peak[tid >> 6] = peak;
        wave_count[tid >> 6] = count;
    }
    __syncthreads();
    int* out = a.partial + ((long long)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kPartial;
    if (tid < 16) out[tid] = cells[tid];
    if (tid == 16) out[16] = max(max(wave_peak[0], wave_peak[1]), max(wave_peak[2], wave_peak[3]));
    if (tid == 17) out[17] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

// one wave per output word: cell (i, j) sums word j of the workgroups of cell row i (a contiguous run of the partials), word 256 is the
// maximum of word 16 of all of them, word 257 the sum of word 17
__global__ __launch_bounds__(256) void frame_difference_reduce_kernel(const int* partial, int per_band, int* out) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= kOutWords) return;
    const int first = o < 256 ? (o >> 4) * per_band : 0;
    const int count = o < 256 ? per_band : 16 * per_band;
    const int word = o < 256 ? (o & 15) : 16 + (o - 256);
    const bool is_max = o == 256;
    int s = 0;                                                // differences are >= 0: the identity of both reductions
    for (int k = lane; k < count; k += 64) {
        const int v = partial[(long long)(first + k) * kPartial + word];
        s = is_max ? max(s, v) : s + v;
    }
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) {
        const int v = __shfl_xor(s, dlt);
        s = is_max ? max(s, v) : s + v;
    }
    if (lane == 0) out[o] = s;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int check_window(const char* what, int h, int w) {
    ATMVFI_REQUIRE(h >= 16 && w >= 16, ATMVFI_EINVAL, "%s: the window must be at least 16 x 16 (got %d x %d)", what, h, w);
    // a cell holds at most ceil(h / 16) * ceil(w / 16) pixels of |difference| <= 255, the count at most h * w pixels
    const long long cell = (long long)((h + 15) / 16) * ((w + 15) / 16);
    ATMVFI_REQUIRE(cell * 255 <= 0x7fffffffll && (long long)h * w <= 0x7fffffffll, ATMVFI_EINVAL,
                   "%s: a %d x %d window is too large (cell sums and the pixel count must fit int32)", what, h, w);
    return ATMVFI_OK;
}

}  // namespace

extern "C" int64_t atmvfi_frame_difference_workspace_ints(int h, int w) {
    if (check_window("frame_difference_workspace_ints", h, w) != ATMVFI_OK) return -1;
    return geometry(h, w).blocks() * kPartial;
}

extern "C" int atmvfi_frame_difference(const void* a, const void* b, int H, int W, int bgr, int y0, int x0, int h, int w, int32_t* out,
                                       int32_t* workspace, int64_t workspace_ints, void* stream) {
    ATMVFI_REQUIRE(a && b && out && workspace, ATMVFI_EINVAL, "frame_difference: null pointer (a %p, b %p, out %p, workspace %p)", a, b,
                   (void*)out, (void*)workspace);
    ATMVFI_REQUIRE(H > 0 && W > 0 && y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && (long long)y0 + h <= H && (long long)x0 + w <= W, ATMVFI_EINVAL,
                   "frame_difference: window outside the frame (%d x %d at (%d, %d) of a %d x %d frame)", h, w, y0, x0, H, W);
    if (const int rc = check_window("frame_difference", h, w)) return rc;
    ATMVFI_REQUIRE(aligned4(out) && aligned4(workspace), ATMVFI_EINVAL, "frame_difference: out and workspace must be 4-byte aligned");
    const DiffGeometry g = geometry(h, w);
    ATMVFI_REQUIRE(workspace_ints >= g.blocks() * kPartial, ATMVFI_EINVAL,
                   "frame_difference: workspace of %lld ints, %lld needed (atmvfi_frame_difference_workspace_ints)", (long long)workspace_ints,
                   g.blocks() * kPartial);
    // aligned path: every lane's 12 bytes of either frame are three dwords and lie inside the window (w % 4 == 0: no group reads past it)
    const bool al = aligned4(a) && aligned4(b) && W % 4 == 0 && x0 % 4 == 0 && w % 4 == 0;
    const DiffArgs args = {(const unsigned char*)a, (const unsigned char*)b, 3ll * W, y0, x0, h, w, g.rows_per_chunk, bgr ? 29 : 77,
                           bgr ? 77 : 29, workspace};
    const dim3 grid((unsigned)g.tiles, (unsigned)g.chunks, 16u), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (al) hipLaunchKernelGGL((frame_difference_partial_kernel<true>), grid, block, 0, st, args);
    else hipLaunchKernelGGL((frame_difference_partial_kernel<false>), grid, block, 0, st, args);
    if (const int rc = atmvfi::check_launch("frame_difference (partials)")) return rc;
    hipLaunchKernelGGL(frame_difference_reduce_kernel, dim3((kOutWords + 3) / 4), block, 0, st, (const int*)workspace, g.tiles * g.chunks, out);
    return atmvfi::check_launch("frame_difference (reduce)");
}
