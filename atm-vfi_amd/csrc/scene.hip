// Frame signature for scene-cut detection in the video loops (include/atmvfi.h, atmvfi_frame_signature; atm-vfi_amd/scene.py): one
// resident uint8 [H,W,3] frame and a window (y0, x0, h, w) -> int32 sig[288]:
//   luma       Y = (77 R + 150 G + 29 B + 128) >> 8            (R is byte 2 of a pixel when `bgr`)
//   sig[16 i + j]  = sum of Y over rows [i h / 16, (i + 1) h / 16) x columns [j w / 16, (j + 1) w / 16)      (16 x 16 cells)
//   sig[256 + b]   = number of window pixels with Y >> 3 == b                                                  (32 bins)
// Integer work only: any reduction order gives the same bits, and the result equals the numpy model (tests/cpu_scene.py) exactly.
//
// Bandwidth-bound and small (6.2 MB at 1080p, 26.5 MB at 4K).  Two launches in one call, no global atomics, nothing to pre-zero:
//   partial kernel: grid (column tiles of 1024 pixels, row chunks, 16 cell rows), 256 lanes.  A lane owns 4 horizontally adjacent
//       pixels (12 contiguous bytes: three dwords on the aligned path, a wave reads 768 contiguous bytes of a row) and walks down the
//       rows of its chunk, 8 rows of loads in flight at a time.  So a lane's four pixel columns -- and with them its cell columns --
//       are fixed: the luma sums stay in four registers for the whole chunk.  The histogram is privatised per workgroup in LDS as
//       [32 bins][32 copies], a lane adding into copy lane % 32: the 32 lanes of an LDS half-group hit 32 different banks whatever
//       their bins are (flat image regions put a whole wave into one bin), and lanes l / l + 32 are served in different groups.
//       At the end the register sums are reduced per wave by a segmented shuffle scan (a lane's cell column is monotone in the lane
//       number), segment heads add into 16 LDS words, and the workgroup writes its 16 + 32 partial words to the caller's workspace.
//   reduce kernel: one wave per output word (288 waves) sums the partials that belong to it and writes sig.
#include "common.h"

namespace {

constexpr int kRows = 8;                 // rows of loads in flight per lane
constexpr int kPartial = 48;             // words per workgroup: 16 cell-column sums of its cell row + 32 bins
constexpr int kTilePixels = 1024;        // 256 lanes x 4 pixels
constexpr long long kMaxBlocks = 4096;

struct alignas(4) U32x3 {
    unsigned a, b, c;
};

struct SigArgs {
    const unsigned char* src;
    long long pitch;        // 3 * W
    int y0, x0, h, w;
    int rows_per_chunk;
    int w0, w2;             // luma weights of bytes 0 and 2 (77 / 29, swapped for BGR)
    int* partial;
};

struct SigGeometry {
    int tiles, chunks, rows_per_chunk;
    long long blocks() const { return 16ll * tiles * chunks; }
};

// the launch geometry of a window; shared by the workspace query and the launch
inline SigGeometry geometry(int h, int w) {
    SigGeometry g;
    g.tiles = (w + kTilePixels - 1) / kTilePixels;
    const int band = (h + 15) / 16;                          // the tallest cell row
    long long rpc = kRows;
    while (rpc < band && 16ll * g.tiles * ((band + rpc - 1) / rpc) > kMaxBlocks) rpc += kRows;
    g.rows_per_chunk = (int)rpc;
    g.chunks = (int)((band + rpc - 1) / rpc);
    return g;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void frame_signature_partial_kernel(const SigArgs a) {
    __shared__ int hist[32 * 32];
    __shared__ int cells[16];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < 32 * 32; k += 256) hist[k] = 0;
    if (tid < 16) cells[tid] = 0;
    __syncthreads();

    const int band = blockIdx.z;
    const int r0 = (int)((long long)band * a.h / 16), r1 = (int)((long long)(band + 1) * a.h / 16);
    const int ya = r0 + blockIdx.y * a.rows_per_chunk;
    const int yb = min(r1, ya + a.rows_per_chunk);
    const int x = blockIdx.x * kTilePixels + tid * 4;         // window column of the lane's first pixel
    int sum[4] = {0, 0, 0, 0};
    int* const myhist = hist + (lane & 31);
    if (x < a.w) {
        const int xl = ALIGNED ? x : min(x, a.w - 1);
        const unsigned char* base = a.src + (long long)a.y0 * a.pitch + (long long)(a.x0 + xl) * 3;
        for (int yy = ya; yy < yb; yy += kRows) {
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
                        if (x + k / 3 < a.w) d[r][k >> 2] |= (unsigned)p[k] << ((k & 3) * 8);
                }
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                if (yy + r < yb) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (x + i < a.w) {
                            const int b0 = (d[r][(3 * i) >> 2] >> (((3 * i) & 3) * 8)) & 0xff;
                            const int b1 = (d[r][(3 * i + 1) >> 2] >> (((3 * i + 1) & 3) * 8)) & 0xff;
                            const int b2 = (d[r][(3 * i + 2) >> 2] >> (((3 * i + 2) & 3) * 8)) & 0xff;
                            const int y = (a.w0 * b0 + 150 * b1 + a.w2 * b2 + 128) >> 8;
                            sum[i] += y;
                            atomicAdd(myhist + (y >> 3) * 32, 1);
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
        int s = sum[i];
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int os = __shfl_down(s, dlt), oj = __shfl_down(j, dlt);
            if (lane + dlt < 64 && oj == j) s += os;
        }
        const int pj = __shfl_up(j, 1);
        if ((lane == 0 || pj != j) && s != 0) atomicAdd(&cells[j], s);
    }
    __syncthreads();
    int* out = a.partial + ((long long)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kPartial;
    if (tid < 16) out[tid] = cells[tid];
    // bin tid / 8: eight lanes sum four copies each, then three shuffles
    int hsum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) hsum += hist[(tid >> 3) * 32 + (tid & 7) * 4 + k];
    hsum += __shfl_xor(hsum, 1);
    hsum += __shfl_xor(hsum, 2);
    hsum += __shfl_xor(hsum, 4);
    if ((tid & 7) == 0) out[16 + (tid >> 3)] = hsum;
}

// one wave per output word: cell (i, j) sums word j of the workgroups of cell row i (a contiguous run of the partials), bin b sums
// word 16 + b of all of them
__global__ __launch_bounds__(256) void frame_signature_reduce_kernel(const int* partial, int per_band, int* sig) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= 288) return;
    const int first = o < 256 ? (o >> 4) * per_band : 0;
    const int count = o < 256 ? per_band : 16 * per_band;
    const int word = o < 256 ? (o & 15) : 16 + (o - 256);
    int s = 0;
    for (int k = lane; k < count; k += 64) s += partial[(long long)(first + k) * kPartial + word];
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) s += __shfl_xor(s, dlt);
    if (lane == 0) sig[o] = s;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int check_window(const char* what, int h, int w) {
    ATMVFI_REQUIRE(h >= 16 && w >= 16, ATMVFI_EINVAL, "%s: the window must be at least 16 x 16 (got %d x %d)", what, h, w);
    // a cell holds at most ceil(h / 16) * ceil(w / 16) pixels of luma <= 255, a bin at most h * w pixels
    const long long cell = (long long)((h + 15) / 16) * ((w + 15) / 16);
    ATMVFI_REQUIRE(cell * 255 <= 0x7fffffffll && (long long)h * w <= 0x7fffffffll, ATMVFI_EINVAL,
                   "%s: a %d x %d window is too large (cell sums and bin counts must fit int32)", what, h, w);
    return ATMVFI_OK;
}

}  // namespace

extern "C" int64_t atmvfi_frame_signature_workspace_ints(int h, int w) {
    if (check_window("frame_signature_workspace_ints", h, w) != ATMVFI_OK) return -1;
    return geometry(h, w).blocks() * kPartial;
}

extern "C" int atmvfi_frame_signature(const void* src, int H, int W, int bgr, int y0, int x0, int h, int w, int32_t* sig, int32_t* workspace,
                                      int64_t workspace_ints, void* stream) {
    ATMVFI_REQUIRE(src && sig && workspace, ATMVFI_EINVAL, "frame_signature: null pointer (src %p, sig %p, workspace %p)", src, (void*)sig,
                   (void*)workspace);
    ATMVFI_REQUIRE(H > 0 && W > 0 && y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && (long long)y0 + h <= H && (long long)x0 + w <= W, ATMVFI_EINVAL,
                   "frame_signature: window outside the frame (%d x %d at (%d, %d) of a %d x %d frame)", h, w, y0, x0, H, W);
    if (const int rc = check_window("frame_signature", h, w)) return rc;
    ATMVFI_REQUIRE(aligned4(sig) && aligned4(workspace), ATMVFI_EINVAL, "frame_signature: sig and workspace must be 4-byte aligned");
    const SigGeometry g = geometry(h, w);
    ATMVFI_REQUIRE(workspace_ints >= g.blocks() * kPartial, ATMVFI_EINVAL,
                   "frame_signature: workspace of %lld ints, %lld needed (atmvfi_frame_signature_workspace_ints)", (long long)workspace_ints,
                   g.blocks() * kPartial);
    // aligned path: every lane's 12 bytes are three dwords and lie inside the window (w % 4 == 0: no group reads past it)
    const bool al = aligned4(src) && W % 4 == 0 && x0 % 4 == 0 && w % 4 == 0;
    const SigArgs a = {(const unsigned char*)src, 3ll * W, y0, x0, h, w, g.rows_per_chunk, bgr ? 29 : 77, bgr ? 77 : 29, workspace};
    const dim3 grid((unsigned)g.tiles, (unsigned)g.chunks, 16u), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (al) hipLaunchKernelGGL((frame_signature_partial_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((frame_signature_partial_kernel<false>), grid, block, 0, st, a);
    if (const int rc = atmvfi::check_launch("frame_signature (partials)")) return rc;
    hipLaunchKernelGGL(frame_signature_reduce_kernel, dim3(72), block, 0, st, (const int*)workspace, g.tiles * g.chunks, sig);
    return atmvfi::check_launch("frame_signature (reduce)");
}
