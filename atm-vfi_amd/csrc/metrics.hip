// Quality metrics of the evaluation scripts: ssim_matlab (benchmark/pytorch_msssim.py:82-135 of the reference) together with the
// squared-error mean of PSNR, for B frame pairs in one call (include/atmvfi.h, atmvfi_ssim_psnr).
//
// ssim_matlab filters [B,1,3,H,W] volumes with an 11x11x11 Gaussian conv3d on replicate-padded inputs.  The window is the outer
// product g x g x g, so the filter is restated separably: along H and W an 11-tap filter with clamped borders, along the 3 channels a
// fixed 3x3 mixing matrix M[o][c] = sum of g[k] over the taps k whose clamped channel c + k - 5 is c.  Filtering is linear, so the
// channel mix runs last, on the 15 filtered quantities (x, y, x*x, y*y, x*y per input channel) of an output pixel only.
//
// One workgroup owns a TILE_H x TILE_W output tile of one sample:
//   1. stage x and y of the tile plus a 5-pixel clamped halo in LDS (6 planes), adding (x - y)^2 of the tile's own pixels to a
//      per-thread fp64 sum on the way (the uint8 ground truth is still at hand there for the fp64 u / 255.0 of PSNR);
//   2. vertical pass: the 15 quantities filtered along H for every halo column, into LDS;
//   3. horizontal pass + channel mix + the SSIM terms in registers, per-thread fp64 sums of ssim_map and v1 / v2;
//   4. a fixed-order LDS tree over the 256 threads; one fp64 partial per sample, statistic and tile goes to the workspace.
// A second kernel sums each sample's partials in a fixed order and writes (or adds) the means.  No floating-point atomics anywhere:
// two runs are bit-identical.  When the value range L is not given, a pre-pass ORs the reference's two conditions on x (max > 128,
// min < -0.5) into an integer word of the workspace; the tile kernel reads it, so there is no host sync.
//
// LDS: every pass walks consecutive columns with consecutive lanes (one b32 per lane, row length 74): conflict-free.
#include "common.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 8, HALO = 5, TAPS = 11;
constexpr int RW = TILE_W + 2 * HALO;           // 74 staged columns
constexpr int RH = TILE_H + 2 * HALO;           // 18 staged rows
constexpr int NT = 256;
constexpr int RAW_FLOATS = 6 * RH * RW;         // x planes 0..2, y planes 3..5
constexpr int V_FLOATS = 15 * TILE_H * RW;      // [quantity][row][column]
constexpr size_t LDS_BYTES = (size_t)(RAW_FLOATS + V_FLOATS) * sizeof(float);
static_assert(RAW_FLOATS * sizeof(float) >= 3 * NT * sizeof(double), "the reduction reuses the staging area");
constexpr int WS_HEAD_FLOATS = 4;               // [0]: range flags (uint32), [1..3]: pad to 16 bytes; fp64 partials follow

struct Weights {
    float g[TAPS];     // normalised 1-D Gaussian, sigma 1.5
    float m[9];        // channel mix M[o * 3 + c]
};

struct Geo {
    long long xb, xc, xy, xx;      // element strides of x (fp32 or uint8)
    long long yb, yc, yy, yx;      // element strides of y (fp32)
    int B, H, W, tiles_x, tiles;
    float val_range;
    int flags;
};

__global__ void __launch_bounds__(NT) ssim_range_kernel(const float* __restrict__ x, Geo g, unsigned* __restrict__ word) {
    const long long hw = (long long)g.H * g.W, total = (long long)g.B * 3 * hw;
    bool hi = false, lo = false;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long bc = i / hw, p = i - bc * hw;
        const long long b = bc / 3, c = bc - b * 3, py = p / g.W, px = p - py * g.W;
        const float v = x[b * g.xb + c * g.xc + py * g.xy + px * g.xx];
        hi |= v > 128.0f;
        lo |= v < -0.5f;
    }
    const int any_hi = __syncthreads_or(hi), any_lo = __syncthreads_or(lo);
    if (threadIdx.x == 0 && (any_hi || any_lo)) atomicOr(word, (any_hi ? 1u : 0u) | (any_lo ? 2u : 0u));
}

__global__ void __launch_bounds__(NT) ssim_tile_kernel(const void* __restrict__ xv, const float* __restrict__ y, Geo g, Weights wt,
                                                       const unsigned* __restrict__ word, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* raw = smem;                      // [6][RH][RW]
    float* vp = smem + RAW_FLOATS;          // [15][TILE_H][RW]
    const int tid = threadIdx.x;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / g.tiles_x) * TILE_H, tx0 = (tile % g.tiles_x) * TILE_W;
    const bool u8 = g.flags & ATMVFI_SSIM_X_U8, bgr = g.flags & ATMVFI_SSIM_X_BGR;
    const bool rnd = g.flags & ATMVFI_SSIM_ROUND_Y, mse32 = g.flags & ATMVFI_SSIM_MSE_F32;
    const unsigned char* xu = static_cast<const unsigned char*>(xv);
    const float* xf = static_cast<const float*>(xv);

    // 1. stage x, y (clamped halo) and the squared error of the tile's own pixels
    double sse = 0.0;
    for (int i = tid; i < RH * RW; i += NT) {
        const int ry = i / RW, rx = i - ry * RW;
        const int oy = ty0 + ry - HALO, ox = tx0 + rx - HALO;
        const int gy = min(max(oy, 0), g.H - 1), gx = min(max(ox, 0), g.W - 1);
        const bool own = ry >= HALO && ry < HALO + TILE_H && rx >= HALO && rx < HALO + TILE_W && oy < g.H && ox < g.W;
        for (int c = 0; c < 3; ++c) {
            const int cx = bgr ? 2 - c : c;
            const long long xo = (long long)b * g.xb + cx * g.xc + (long long)gy * g.xy + (long long)gx * g.xx;
            float xs, yv = y[(long long)b * g.yb + c * g.yc + (long long)gy * g.yy + (long long)gx * g.yx];
            double xd;
            if (u8) {
                const unsigned u = xu[xo];
                xs = (float)u / 255.0f;
                xd = (double)u / 255.0;
            } else {
                xs = xf[xo];
                xd = (double)xs;
            }
            if (rnd) yv = rintf(yv * 255.0f) / 255.0f;
            if (own) {
                if (mse32) {
                    const float d = xs - yv;
                    sse += (double)(d * d);
                } else {
                    const double d = xd - (double)yv;
                    sse += d * d;
                }
            }
            raw[(c * RH + ry) * RW + rx] = xs;
            raw[((3 + c) * RH + ry) * RW + rx] = yv;
        }
    }
    __syncthreads();

    // 2. vertical pass: x, y, xx, yy, xy of every input channel filtered along H
    for (int i = tid; i < TILE_H * RW; i += NT) {
        const int r = i / RW, j = i - r * RW;
        for (int c = 0; c < 3; ++c) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                const float w = wt.g[k];
                const float xs = raw[(c * RH + r + k) * RW + j], ys = raw[((3 + c) * RH + r + k) * RW + j];
                a0 += w * xs;
                a1 += w * ys;
                a2 += w * (xs * xs);
                a3 += w * (ys * ys);
                a4 += w * (xs * ys);
            }
            vp[((c * 5 + 0) * TILE_H + r) * RW + j] = a0;
            vp[((c * 5 + 1) * TILE_H + r) * RW + j] = a1;
            vp[((c * 5 + 2) * TILE_H + r) * RW + j] = a2;
            vp[((c * 5 + 3) * TILE_H + r) * RW + j] = a3;
            vp[((c * 5 + 4) * TILE_H + r) * RW + j] = a4;
        }
    }

    // value range and constants (the reference's Python doubles, used in fp32 arithmetic)
    double L = g.val_range;
    if (!(g.val_range > 0.0f)) {
        if (u8) {
            L = 1.0;               // u / 255 lies in [0, 1]
        } else {
            const unsigned f = *word;
            L = ((f & 1u) ? 255.0 : 1.0) - ((f & 2u) ? -1.0 : 0.0);
        }
    }
    const float C1 = (float)((0.01 * L) * (0.01 * L)), C2 = (float)((0.03 * L) * (0.03 * L));
    __syncthreads();

    // 3. horizontal pass, channel mix, SSIM terms
    double s_ssim = 0.0, s_cs = 0.0;
    const int col = tid % TILE_W;
    for (int r = tid / TILE_W; r < TILE_H; r += NT / TILE_W) {
        if (ty0 + r >= g.H || tx0 + col >= g.W) continue;
        float h[15];
#pragma unroll
        for (int q = 0; q < 15; ++q) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) a += wt.g[k] * vp[(q * TILE_H + r) * RW + col + k];
            h[q] = a;
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            float f[5];
#pragma unroll
            for (int s = 0; s < 5; ++s) f[s] = wt.m[o * 3 + 0] * h[s] + wt.m[o * 3 + 1] * h[5 + s] + wt.m[o * 3 + 2] * h[10 + s];
            const float mu1 = f[0], mu2 = f[1];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const float s1 = f[2] - mu1_sq, s2 = f[3] - mu2_sq, s12 = f[4] - mu1_mu2;
            const float v1 = 2.0f * s12 + C2, v2 = s1 + s2 + C2;
            s_cs += (double)(v1 / v2);
            s_ssim += (double)(((2.0f * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2));
        }
    }
    __syncthreads();          // the staging area becomes the reduction's

    // 4. fixed-order reduction over the workgroup
    double* red = reinterpret_cast<double*>(smem);
    red[tid] = s_ssim;
    red[NT + tid] = s_cs;
    red[2 * NT + tid] = sse;
    __syncthreads();
    for (int n = NT / 2; n > 0; n >>= 1) {
        if (tid < n) {
            red[tid] += red[tid + n];
            red[NT + tid] += red[NT + tid + n];
            red[2 * NT + tid] += red[2 * NT + tid + n];
        }
        __syncthreads();
    }
    if (tid < 3) part[((long long)b * 3 + tid) * g.tiles + tile] = red[tid * NT];
}

__global__ void __launch_bounds__(NT) ssim_final_kernel(const double* __restrict__ part, Geo g, double* __restrict__ out) {
    __shared__ double red[3][NT];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int s = 0; s < 3; ++s) {
        double a = 0.0;
        for (int t = tid; t < g.tiles; t += NT) a += part[((long long)b * 3 + s) * g.tiles + t];
        red[s][tid] = a;
    }
    __syncthreads();
    for (int n = NT / 2; n > 0; n >>= 1) {
        if (tid < n)
            for (int s = 0; s < 3; ++s) red[s][tid] += red[s][tid + n];
        __syncthreads();
    }
    if (tid < 3) {
        const double v = red[tid][0] / (3.0 * g.H * g.W);
        if (g.flags & ATMVFI_SSIM_ACCUMULATE)
            out[b * 3 + tid] += v;
        else
            out[b * 3 + tid] = v;
    }
}

int tiles_of(int H, int W) { return ((H + TILE_H - 1) / TILE_H) * ((W + TILE_W - 1) / TILE_W); }

Weights make_weights() {
    // gaussian(11, 1.5) of the reference: fp32 of exp(-(k-5)^2 / 4.5), divided by its fp32 sum
    Weights w;
    float sum = 0.f;
    for (int k = 0; k < TAPS; ++k) {
        w.g[k] = (float)exp(-(double)((k - 5) * (k - 5)) / 4.5);
        sum += w.g[k];
    }
    for (int k = 0; k < TAPS; ++k) w.g[k] /= sum;
    for (int o = 0; o < 3; ++o)
        for (int c = 0; c < 3; ++c) {
            float m = 0.f;
            for (int k = 0; k < TAPS; ++k)
                if ((o + k - HALO < 0 ? 0 : o + k - HALO > 2 ? 2 : o + k - HALO) == c) m += w.g[k];
            w.m[o * 3 + c] = m;
        }
    return w;
}

}  // namespace

extern "C" int64_t atmvfi_ssim_psnr_workspace_floats(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return WS_HEAD_FLOATS + (int64_t)B * 3 * tiles_of(H, W) * 2;
}

extern "C" int atmvfi_ssim_psnr(const void* x, int64_t x_bstride, int64_t x_cstride, int64_t x_ystride, int64_t x_xstride, const float* y,
                                int64_t y_bstride, int64_t y_cstride, int64_t y_ystride, int64_t y_xstride, int B, int H, int W,
                                float val_range, int flags, double* out, float* workspace, int64_t workspace_floats, void* stream) {
    ATMVFI_REQUIRE(x && y && out && workspace, ATMVFI_EINVAL, "ssim_psnr: null pointer");
    ATMVFI_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, ATMVFI_EINVAL, "ssim_psnr: bad shape (B %d, H %d, W %d)", B, H, W);
    ATMVFI_REQUIRE(H >= TAPS && W >= TAPS, ATMVFI_EINVAL,
                   "ssim_psnr: H and W must be at least 11 (got %dx%d); the reference shrinks its window below that, which is not supported",
                   H, W);
    ATMVFI_REQUIRE((flags & ~ATMVFI_SSIM_FLAG_MASK) == 0, ATMVFI_EINVAL, "ssim_psnr: unknown flag bits 0x%x", flags);
    ATMVFI_REQUIRE(x_bstride >= 0 && x_cstride >= 0 && x_ystride >= 0 && x_xstride >= 0 && y_bstride >= 0 && y_cstride >= 0 &&
                       y_ystride >= 0 && y_xstride >= 0,
                   ATMVFI_EINVAL, "ssim_psnr: negative stride");
    ATMVFI_REQUIRE(((uintptr_t)out & 7u) == 0 && atmvfi::aligned16(workspace), ATMVFI_EALIGN,
                   "ssim_psnr: out must be 8-byte and the workspace 16-byte aligned");
    const int64_t need = atmvfi_ssim_psnr_workspace_floats(B, H, W);
    ATMVFI_REQUIRE(workspace_floats >= need, ATMVFI_EINVAL,
                   "ssim_psnr: needs a workspace of atmvfi_ssim_psnr_workspace_floats(B, H, W) = %lld floats (got %lld)", (long long)need,
                   (long long)workspace_floats);
    static const Weights wt = make_weights();
    Geo g;
    g.xb = x_bstride; g.xc = x_cstride; g.xy = x_ystride; g.xx = x_xstride;
    g.yb = y_bstride; g.yc = y_cstride; g.yy = y_ystride; g.yx = y_xstride;
    g.B = B; g.H = H; g.W = W;
    g.tiles_x = (W + TILE_W - 1) / TILE_W;
    g.tiles = tiles_of(H, W);
    g.val_range = val_range;
    g.flags = flags;
    const hipStream_t s = (hipStream_t)stream;
    unsigned* word = reinterpret_cast<unsigned*>(workspace);
    double* part = reinterpret_cast<double*>(workspace + WS_HEAD_FLOATS);
    if (!(val_range > 0.0f) && !(flags & ATMVFI_SSIM_X_U8)) {
        const hipError_t e = hipMemsetAsync(word, 0, sizeof(unsigned), s);
        ATMVFI_REQUIRE(e == hipSuccess, ATMVFI_ELAUNCH, "ssim_psnr: hipMemsetAsync: %s", hipGetErrorString(e));
        const long long total = (long long)B * 3 * H * W;
        const long long blocks = (total + NT * 8 - 1) / (NT * 8);
        hipLaunchKernelGGL(ssim_range_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(NT), 0, s,
                           static_cast<const float*>(x), g, word);
    }
    const hipError_t attr = atmvfi::allow_dynamic_lds<ssim_tile_kernel>(LDS_BYTES);
    ATMVFI_REQUIRE(attr == hipSuccess, ATMVFI_ELAUNCH, "ssim_psnr: hipFuncSetAttribute: %s", hipGetErrorString(attr));
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)g.tiles, (unsigned)B), dim3(NT), LDS_BYTES, s, x, y, g, wt, word, part);
    hipLaunchKernelGGL(ssim_final_kernel, dim3((unsigned)B), dim3(NT), 0, s, part, g, out);
    return atmvfi::check_launch("ssim_psnr");
}
