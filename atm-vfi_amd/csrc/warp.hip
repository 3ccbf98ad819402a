// The image-geometry kernels of the ATM-VFI hot path for gfx950: backward bilinear warps (direct gathers and LDS-staged tiles), the
// fused warp/blend synthesis, the align_corners resize, the image pyramid and the frame pack.  HBM-bound, one pass each.  Shared pieces
// stand here once: the taps (make_taps, with a padding map for flow_warp_ex), the tile walk (warp_tile), the align_corners bilinear
// (ac_taps / ac_blend), the x2 flow up-sampling (flow_up2_element), the frame pack (pack_frame_element) and the launchers' checks.
// Three things still stand more than once, because every shared form that was compiled changed the direct kernels' device code and
// measured slower than the parent (profiles/warp_fold_ab.txt):
//   - the per-pixel index / flow / channel loop of flow_warp_planar, flow_warp_ex and the warp half of flow_warp_up2 (6 lines each);
//   - the body of warp_blend_kernel and warp_blend_tiled_kernel after the sampling (flows, masks, pack15, plane sink: 45 lines each);
//   - flow_up2_geometry writes the x2 scale without ac_scale's `out > 1` select (one VGPR in flow_warp_up2).
// tests/test_gpu_ops.py holds the kernels that repeat a piece to each other's bits.
#include "common.h"

#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------
// Sampling coordinates exactly as the reference computes them (flow_warp.py:35-36 normalise,
// then grid_sample(align_corners=True) un-normalises): the round trip is kept so that the
// tap positions are bit-identical to the reference's.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float norm_coord(float p, int size) { return 2.0f * p / (float)(size - 1) - 1.0f; }
__device__ __forceinline__ float ref_coord(float p, int size) { return ((norm_coord(p, size) + 1.0f) / 2.0f) * (float)(size - 1); }

struct Taps {
    int x0, y0;
    float w00, w01, w10, w11;   // (y0,x0) (y0,x1) (y1,x0) (y1,x1); zero when the tap is outside
    bool in00, in01, in10, in11;
};

// The four taps around pixel position (px, py), zero padding: a tap outside the image has no weight.  pad(coordinate, size) maps the
// un-normalised coordinate first (flow_warp_ex's border / reflection modes); every other warp takes the coordinate as it is.
struct NoPad {
    __device__ __forceinline__ float operator()(float c, int) const { return c; }
};
template <class Pad = NoPad>
__device__ __forceinline__ Taps make_taps(float px, float py, int W, int H, Pad pad = Pad()) {
    Taps t;
    const float ix = pad(ref_coord(px, W), W), iy = pad(ref_coord(py, H), H);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    // clamp before the int conversion so wild flows cannot overflow
    const float cx = fminf(fmaxf(fx0, -2.0f), (float)W + 1.0f), cy = fminf(fmaxf(fy0, -2.0f), (float)H + 1.0f);
    t.x0 = (int)cx;
    t.y0 = (int)cy;
    const float ax = ix - fx0, ay = iy - fy0;   // weight of the +1 neighbour
    const bool far = (cx != fx0) || (cy != fy0) || !(ix == ix) || !(iy == iy);
    t.in00 = !far && t.x0 >= 0 && t.x0 < W && t.y0 >= 0 && t.y0 < H;
    t.in01 = !far && t.x0 + 1 >= 0 && t.x0 + 1 < W && t.y0 >= 0 && t.y0 < H;
    t.in10 = !far && t.x0 >= 0 && t.x0 < W && t.y0 + 1 >= 0 && t.y0 + 1 < H;
    t.in11 = !far && t.x0 + 1 >= 0 && t.x0 + 1 < W && t.y0 + 1 >= 0 && t.y0 + 1 < H;
    t.w00 = (1.0f - ax) * (1.0f - ay);
    t.w01 = ax * (1.0f - ay);
    t.w10 = (1.0f - ax) * ay;
    t.w11 = ax * ay;
    return t;
}

__device__ __forceinline__ float sample_plane(const float* __restrict__ p, const Taps& t, int W) {
    float v = 0.f;
    const float* b = p + (long long)t.y0 * W + t.x0;
    if (t.in00) v += b[0] * t.w00;
    if (t.in01) v += b[1] * t.w01;
    if (t.in10) v += b[W] * t.w10;
    if (t.in11) v += b[W + 1] * t.w11;
    return v;
}

__global__ __launch_bounds__(256) void flow_warp_planar_kernel(const float* __restrict__ src, const float* __restrict__ flow,
                                                               long long flow_bstride, int flow_pstride, int flow_cstride,
                                                               float* __restrict__ dst, int B, int C, int H, int W) {
    fp16_saturate_on();
    const long long hw = (long long)H * W;
    const long long total = (long long)B * hw;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(idx / hw);
        const long long pix = idx - (long long)b * hw;
        const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
        const float* fp = flow + b * flow_bstride + pix * flow_pstride;
        const Taps t = make_taps((float)x + fp[0], (float)y + fp[flow_cstride], W, H);
        for (int c = 0; c < C; ++c)
            dst[((long long)b * C + c) * hw + pix] = sample_plane(src + ((long long)b * C + c) * hw, t, W);
    }
}

// The non-default forms of the reference's flow_warp (flow_warp.py:50-60 -> bilinear_sample :26-47): padding_mode 'border' /
// 'reflection' (grid_sample's coordinate maps for align_corners=True: clip to [0, size-1]; reflect about 0 and size-1, then clip)
// and return_mask (the normalised coordinate inside [-1, 1] on both axes, evaluated on the reference's own fp32 expression
// 2 p / (size - 1) - 1, so that a coordinate a rounding below zero is "inside" exactly when the reference says so).  Off the hot path:
// one lane per pixel, direct gathers.  mode: 0 zeros, 1 border, 2 reflection.
__device__ __forceinline__ float pad_coord(float c, int size, int mode) {
    if (mode == 0) return c;
    const float hi = (float)(size - 1);
    if (mode == 2) {                                         // reflect_coordinates(c, 0, 2 (size - 1)) of ATen's GridSampler.h
        if (size == 1) c = 0.f;
        else {
            const float a = fabsf(c), extra = fmodf(a, hi);
            const int flips = (int)floorf(a / hi);
            c = (flips & 1) ? hi - extra : extra;
        }
    }
    return fminf(hi, fmaxf(c, 0.f));                         // clip_coordinates
}
__global__ __launch_bounds__(256) void flow_warp_ex_kernel(const float* __restrict__ src, const float* __restrict__ flow, float* __restrict__ dst,
                                                           unsigned char* __restrict__ mask, int B, int C, int H, int W, int mode) {
    fp16_saturate_on();
    const long long hw = (long long)H * W;
    const long long total = (long long)B * hw;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(idx / hw);
        const long long pix = idx - (long long)b * hw;
        const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
        const float* fp = flow + (long long)b * 2 * hw + pix;
        const float px = (float)x + fp[0], py = (float)y + fp[hw];
        const float gx = norm_coord(px, W), gy = norm_coord(py, H);
        if (mask) mask[idx] = (gx >= -1.0f) && (gy >= -1.0f) && (gx <= 1.0f) && (gy <= 1.0f);
        const Taps t = make_taps(px, py, W, H, [mode](float c, int size) { return pad_coord(c, size, mode); });
        for (int c = 0; c < C; ++c)
            dst[((long long)b * C + c) * hw + pix] = sample_plane(src + ((long long)b * C + c) * hw, t, W);
    }
}

// ---------------------------------------------------------------------------------------
// align_corners=True bilinear (ATen upsample_bilinear2d arithmetic): the source position and weights of one output element, and the
// blend of its four source values.  The resize, the x2 flow up-sampling and the pyramid differ only in how they fetch the four.
// ---------------------------------------------------------------------------------------
struct AcTaps {
    int y0, x0, yp, xp;         // the taps are (y0, x0), (y0, x0 + xp), (y0 + yp, x0), (y0 + yp, x0 + xp)
    float ly, lx, hy, hx;
};
__device__ __forceinline__ float ac_scale(int in, int out) { return (out > 1) ? (float)(in - 1) / (float)(out - 1) : 0.f; }
__device__ __forceinline__ AcTaps ac_taps(float sh, float sw, int oy, int ox, int Hi, int Wi) {
    AcTaps a;
    const float ry = sh * (float)oy, rx = sw * (float)ox;
    a.y0 = (int)ry;
    a.x0 = (int)rx;
    a.yp = (a.y0 < Hi - 1) ? 1 : 0;
    a.xp = (a.x0 < Wi - 1) ? 1 : 0;
    a.ly = ry - (float)a.y0;
    a.lx = rx - (float)a.x0;
    a.hy = 1.0f - a.ly;
    a.hx = 1.0f - a.lx;
    return a;
}
__device__ __forceinline__ float ac_blend(const AcTaps& a, float v00, float v01, float v10, float v11) {
    return a.hy * (a.hx * v00 + a.lx * v01) + a.ly * (a.hx * v10 + a.lx * v11);
}

// The x2 up-sampling of a B x 2 x H x W flow (upsample_flow, network_base.py:11-18: bilinear, align_corners=True, values x 2): its
// geometry, computed once per kernel, and element e of the B x 2 x 2H x 2W output
struct FlowUp2 {
    int Wo;
    long long ohw;
    float sh, sw;
};
__device__ __forceinline__ FlowUp2 flow_up2_geometry(int H, int W) {
    const int Ho = 2 * H, Wo = 2 * W;
    return FlowUp2{Wo, (long long)Ho * Wo, (float)(H - 1) / (float)(Ho - 1), (float)(W - 1) / (float)(Wo - 1)};     // ac_scale: Ho, Wo > 1
}
__device__ __forceinline__ void flow_up2_element(const float* __restrict__ flow, float* __restrict__ flow_up, const FlowUp2& u, long long e, int H,
                                                 int W) {
    const int p = (int)(e / u.ohw);                  // plane b * 2 + c
    const long long pix = e - (long long)p * u.ohw;
    const int oy = (int)(pix / u.Wo), ox = (int)(pix - (long long)oy * u.Wo);
    const AcTaps a = ac_taps(u.sh, u.sw, oy, ox, H, W);
    const float* s = flow + (long long)p * ((long long)H * W) + (long long)a.y0 * W + a.x0;
    const float v = ac_blend(a, s[0], s[a.xp], s[a.yp * W], s[a.yp * W + a.xp]);
    flow_up[e] = v * 2.0f;
}

// flow_warp of a planar image by a planar flow AND the x2 up-sampling of that flow to the next finer level in one launch: the global
// flow's walk down the image pyramid (network_base.py:468-485) is four warps and three up-samplings in a chain.  The two halves of the
// index space are independent: flow_warp_planar_kernel's pixel and flow_up2_element, bit-identical to a flow_warp and a resize launch.
__global__ __launch_bounds__(256) void flow_warp_up2_kernel(const float* __restrict__ src, const float* __restrict__ flow, float* __restrict__ dst,
                                                            float* __restrict__ flow_up, int B, int C, int H, int W) {
    fp16_saturate_on();
    const long long hw = (long long)H * W;
    const long long nwarp = (long long)B * hw;
    const FlowUp2 u = flow_up2_geometry(H, W);
    const long long nup = (long long)B * 2 * u.ohw;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < nwarp + nup; idx += (long long)gridDim.x * blockDim.x) {
        if (idx < nwarp) {
            const int b = (int)(idx / hw);
            const long long pix = idx - (long long)b * hw;
            const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
            const float* fp = flow + (long long)b * 2 * hw + pix;
            const Taps t = make_taps((float)x + fp[0], (float)y + fp[hw], W, H);
            for (int c = 0; c < C; ++c)
                dst[((long long)b * C + c) * hw + pix] = sample_plane(src + ((long long)b * C + c) * hw, t, W);
        } else flow_up2_element(flow, flow_up, u, idx - nwarp, H, W);
    }
}

__global__ __launch_bounds__(256) void flow_warp_nhwc_kernel(const float* __restrict__ src, int src_ld, long long src_bstride,
                                                             const float* __restrict__ flow, long long flow_bstride,
                                                             int flow_pstride, int flow_cstride, float* __restrict__ dst,
                                                             int dst_ld, long long dst_bstride, int B, int C, int H, int W) {
    fp16_saturate_on();
    const int c4n = C >> 2;
    const long long hw = (long long)H * W;
    const long long total = (long long)B * hw * c4n;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) << 2;
        const long long bp = idx / c4n;
        const int b = (int)(bp / hw);
        const long long pix = bp - (long long)b * hw;
        const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
        const float* fp = flow + b * flow_bstride + pix * flow_pstride;
        const Taps t = make_taps((float)x + fp[0], (float)y + fp[flow_cstride], W, H);
        const float* sb = src + b * src_bstride + ((long long)t.y0 * W + t.x0) * src_ld + c;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (t.in00) { const f32x4 v = *reinterpret_cast<const f32x4*>(sb); acc += v * t.w00; }
        if (t.in01) { const f32x4 v = *reinterpret_cast<const f32x4*>(sb + src_ld); acc += v * t.w01; }
        if (t.in10) { const f32x4 v = *reinterpret_cast<const f32x4*>(sb + (long long)W * src_ld); acc += v * t.w10; }
        if (t.in11) { const f32x4 v = *reinterpret_cast<const f32x4*>(sb + (long long)(W + 1) * src_ld); acc += v * t.w11; }
        *reinterpret_cast<f32x4*>(dst + b * dst_bstride + pix * dst_ld + c) = acc;
    }
}

// ---------------------------------------------------------------------------------------
// fused synthesis at one pyramid level: the two flows and the mask of a pixel, then its warps, blend and outputs
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void warp_blend_kernel(const float* __restrict__ im0, const float* __restrict__ im1,
                                                         const float* __restrict__ motion, int motion_ld, long long motion_bstride,
                                                         float* __restrict__ i0w, float* __restrict__ i1w, float* __restrict__ it,
                                                         float* __restrict__ f0o, float* __restrict__ f1o,
                                                         float* __restrict__ m1o, float* __restrict__ m2o,
                                                         const float* __restrict__ orig0, const float* __restrict__ orig1,
                                                         float* __restrict__ pack15, int pack_ld, _Float16* __restrict__ pack_hi,
                                                         _Float16* __restrict__ pack_lo, long long pack_rows, int pack_c0, int B, int H,
                                                         int W) {
    fp16_saturate_on();
    const long long hw = (long long)H * W;
    const long long total = (long long)B * hw;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(idx / hw);
        const long long pix = idx - (long long)b * hw;
        const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
        const float* mp = motion + b * motion_bstride + pix * motion_ld;
        const float fx0 = mp[0], fy0 = mp[1], fx1 = mp[2], fy1 = mp[3];
        const float m1 = sigmoidf_(mp[4]);
        const float m2 = 1.0f - m1;
        const Taps t0 = make_taps((float)x + fx0, (float)y + fy0, W, H);
        const Taps t1 = make_taps((float)x + fx1, (float)y + fy1, W, H);
        float a[3], c[3], o[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long pl = ((long long)b * 3 + ch) * hw;
            a[ch] = sample_plane(im0 + pl, t0, W);
            c[ch] = sample_plane(im1 + pl, t1, W);
            o[ch] = m1 * a[ch] + m2 * c[ch];
            i0w[pl + pix] = a[ch];
            i1w[pl + pix] = c[ch];
            it[pl + pix] = o[ch];
        }
        if (f0o) {
            f0o[((long long)b * 2) * hw + pix] = fx0;
            f0o[((long long)b * 2 + 1) * hw + pix] = fy0;
            f1o[((long long)b * 2) * hw + pix] = fx1;
            f1o[((long long)b * 2 + 1) * hw + pix] = fy1;
        }
        if (m1o) {
            m1o[(long long)b * hw + pix] = m1;
            m2o[(long long)b * hw + pix] = m2;
        }
        if (pack15) {
            float* pp = pack15 + ((long long)b * hw + pix) * pack_ld;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const long long pl = ((long long)b * 3 + ch) * hw + pix;
                pp[ch] = orig0[pl];
                pp[3 + ch] = a[ch];
                pp[6 + ch] = orig1[pl];
                pp[9 + ch] = c[ch];
                pp[12 + ch] = o[ch];
            }
        }
        if (pack_hi) {
            // the same 15 values (+ one zero) as split planes at channels pack_c0 .. pack_c0 + 16: the refiner's first conv reads
            // its input as planes (atmvfi_conv3x3_planes)
            float v16[16];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const long long pl = ((long long)b * 3 + ch) * hw + pix;
                v16[ch] = orig0[pl];
                v16[3 + ch] = a[ch];
                v16[6 + ch] = orig1[pl];
                v16[9 + ch] = c[ch];
                v16[12 + ch] = o[ch];
            }
            v16[15] = 0.f;
            const RowSink sink{nullptr, 0, pack_hi, pack_lo, pack_rows};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                sink_store4(sink, (long long)b * hw + pix, pack_c0 + 4 * q, (f32x4){v16[4 * q], v16[4 * q + 1], v16[4 * q + 2], v16[4 * q + 3]});
        }
    }
}

// ---------------------------------------------------------------------------------------
// The same warps with LDS-STAGED SOURCE TILES (the north star's form of flow_warp.py:50-60): a workgroup owns a 32 x 8 tile of output
// pixels; it reduces the bounding box of its lanes' bilinear taps (cross-lane minima, one LDS atomic per wave), loads that box of every source plane with
// 16-byte row loads into LDS (up to 64 x 24 source pixels: flows of about +-15 px horizontally, +-8 vertically around the tile) and
// takes the four taps of every pixel from LDS -- ~5 coalesced dwordx4 loads per lane and source instead of 12 gathered dwords.  A tile
// whose flows reach further than the box gathers from global memory as the direct kernels do (a workgroup-uniform decision, per
// source).  Taps, weights and the order of the four multiply-adds are those of sample_plane: results are bit-identical to the direct
// kernels (tests/test_gpu_ops.py::test_tiled_warps_equal_direct_warps).  Needs W % 4 == 0 and 16-byte aligned planes.
// ---------------------------------------------------------------------------------------
constexpr int WT_W = 32, WT_H = 8;            // output tile of a workgroup (256 lanes)
constexpr int WB_W = 64, WB_H = 24;           // staged box per source plane, pixels
constexpr int WB_PLANE = WB_W * WB_H;

struct StagedBox {
    int ax0, y0, nv, h;      // columns ax0 .. ax0 + 4 nv - 1 (ax0 a multiple of 4), rows y0 .. y0 + h - 1
    bool ok;                 // it fits the LDS box (an empty box -- no live tap in the tile -- counts as staged)
};

__device__ __forceinline__ void box_reset(int* bx) {       // {x lo, x hi, y lo, y hi}
    bx[0] = 0x7fffffff; bx[1] = -0x7fffffff; bx[2] = 0x7fffffff; bx[3] = -0x7fffffff;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const int u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}
__device__ __forceinline__ void box_add(int* bx, const Taps& t, bool live, int W, int H) {
    // the wave's extremes by cross-lane exchange, then one LDS atomic per wave and bound (64 lanes on one LDS word serialise)
    const bool any = live && (t.in00 || t.in01 || t.in10 || t.in11);      // some tap inside the image: x0 in [-1, W-1], y0 in [-1, H-1]
    const int xlo = any ? (t.x0 < 0 ? 0 : t.x0) : 0x7fffffff;
    const int xhi = any ? (t.x0 + 1 > W - 1 ? W - 1 : t.x0 + 1) : -0x7fffffff;
    const int ylo = any ? (t.y0 < 0 ? 0 : t.y0) : 0x7fffffff;
    const int yhi = any ? (t.y0 + 1 > H - 1 ? H - 1 : t.y0 + 1) : -0x7fffffff;
    const int a = wave_min_i32(xlo), b = -wave_min_i32(-xhi), c = wave_min_i32(ylo), d = -wave_min_i32(-yhi);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&bx[0], a);
        atomicMax(&bx[1], b);
        atomicMin(&bx[2], c);
        atomicMax(&bx[3], d);
    }
}
__device__ __forceinline__ StagedBox box_get(const int* bx) {
    StagedBox b;
    if (bx[0] > bx[1]) { b.ax0 = 0; b.y0 = 0; b.nv = 0; b.h = 0; b.ok = true; return b; }
    b.ax0 = bx[0] & ~3;
    b.y0 = bx[2];
    b.nv = ((bx[1] - b.ax0) >> 2) + 1;
    b.h = bx[3] - bx[2] + 1;
    b.ok = b.nv <= WB_W / 4 && b.h <= WB_H;
    return b;
}
// nch planes (plane stride hw floats) of the box into tile[ch][row][WB_W]; all 256 lanes of the workgroup take part
__device__ __forceinline__ void box_stage(float* tile, const float* __restrict__ src, long long hw, int W, int nch, const StagedBox& b, int tid) {
    const int per = b.h * b.nv, total = nch * per;
    for (int i = tid; i < total; i += 256) {
        const int ch = i / per, rem = i - ch * per;
        const int r = rem / b.nv, v = rem - r * b.nv;
        const f32x4 q = *reinterpret_cast<const f32x4*>(src + ch * hw + (long long)(b.y0 + r) * W + b.ax0 + 4 * v);
        *reinterpret_cast<f32x4*>(tile + ch * WB_PLANE + r * WB_W + 4 * v) = q;
    }
}
__device__ __forceinline__ float sample_tile(const float* tile_plane, const Taps& t, const StagedBox& b) {
    float v = 0.f;
    const float* p = tile_plane + (t.y0 - b.y0) * WB_W + (t.x0 - b.ax0);
    if (t.in00) v += p[0] * t.w00;
    if (t.in01) v += p[1] * t.w01;
    if (t.in10) v += p[WB_W] * t.w10;
    if (t.in11) v += p[WB_W + 1] * t.w11;
    return v;
}
// tile origin of this workgroup: blockIdx.x = (b * tiles_y + ty) * tiles_x + tx
__device__ __forceinline__ void tile_pixel(int H, int W, int& b, int& x, int& y, bool& live) {
    const int tiles_x = (W + WT_W - 1) / WT_W, tiles_y = (H + WT_H - 1) / WT_H;
    const int t = blockIdx.x, tx = t % tiles_x, r = t / tiles_x;
    b = r / tiles_y;
    x = tx * WT_W + (threadIdx.x & (WT_W - 1));
    y = (r - b * tiles_y) * WT_H + (threadIdx.x >> 5);
    live = x < W && y < H;
}

// flow_warp of this workgroup's tile (tile_pixel), every channel, three planes staged at a time; tile: 3 * WB_PLANE floats, bx: 4 ints
__device__ __forceinline__ void warp_tile(float* tile, int* bx, const float* __restrict__ src, const float* __restrict__ flow, long long flow_bstride,
                                          int flow_pstride, long long flow_cstride, float* __restrict__ dst, int C, int H, int W) {
    const int tid = threadIdx.x;
    const long long hw = (long long)H * W;
    int b, x, y;
    bool live;
    tile_pixel(H, W, b, x, y, live);
    const long long pix = (long long)(live ? y : 0) * W + (live ? x : 0);
    if (tid == 0) box_reset(bx);
    const float* fp = flow + b * flow_bstride + pix * flow_pstride;
    const Taps t = make_taps((float)x + fp[0], (float)y + fp[flow_cstride], W, H);
    __syncthreads();
    box_add(bx, t, live, W, H);
    __syncthreads();
    const StagedBox sb = box_get(bx);
    for (int c0 = 0; c0 < C; c0 += 3) {
        const int nch = C - c0 < 3 ? C - c0 : 3;
        const float* sp = src + ((long long)b * C + c0) * hw;
        if (sb.ok) {
            if (c0) __syncthreads();                         // the previous group's taps have been read
            box_stage(tile, sp, hw, W, nch, sb, tid);
            __syncthreads();
        }
        if (live)
            for (int c = 0; c < nch; ++c)
                dst[((long long)b * C + c0 + c) * hw + pix] = sb.ok ? sample_tile(tile + c * WB_PLANE, t, sb) : sample_plane(sp + c * hw, t, W);
    }
}

__global__ __launch_bounds__(256) void flow_warp_tiled_kernel(const float* __restrict__ src, const float* __restrict__ flow,
                                                              long long flow_bstride, int flow_pstride, int flow_cstride,
                                                              float* __restrict__ dst, int B, int C, int H, int W) {
    fp16_saturate_on();
    __shared__ __attribute__((aligned(16))) float tile[3 * WB_PLANE];
    __shared__ int bx[4];
    warp_tile(tile, bx, src, flow, flow_bstride, flow_pstride, flow_cstride, dst, C, H, W);
}

// flow_warp_up2_kernel with the warp half on LDS-staged tiles: workgroups 0 .. ntiles-1 warp one 32 x 8 tile each (warp_tile), the
// others up-sample the flow (grid-stride over the 2 B x 2H x 2W outputs)
__global__ __launch_bounds__(256) void flow_warp_up2_tiled_kernel(const float* __restrict__ src, const float* __restrict__ flow, float* __restrict__ dst,
                                                                  float* __restrict__ flow_up, int B, int C, int H, int W, int ntiles) {
    fp16_saturate_on();
    __shared__ __attribute__((aligned(16))) float tile[3 * WB_PLANE];
    __shared__ int bx[4];
    const long long hw = (long long)H * W;
    if ((int)blockIdx.x < ntiles) {
        warp_tile(tile, bx, src, flow, 2 * hw, 1, hw, dst, C, H, W);
        return;
    }
    const FlowUp2 u = flow_up2_geometry(H, W);
    const long long nup = (long long)B * 2 * u.ohw;
    for (long long e = (long long)(blockIdx.x - ntiles) * blockDim.x + threadIdx.x; e < nup; e += (long long)(gridDim.x - ntiles) * blockDim.x)
        flow_up2_element(flow, flow_up, u, e, H, W);
}

__global__ __launch_bounds__(256) void warp_blend_tiled_kernel(const float* __restrict__ im0, const float* __restrict__ im1,
                                                               const float* __restrict__ motion, int motion_ld, long long motion_bstride,
                                                               float* __restrict__ i0w, float* __restrict__ i1w, float* __restrict__ it,
                                                               float* __restrict__ f0o, float* __restrict__ f1o,
                                                               float* __restrict__ m1o, float* __restrict__ m2o,
                                                               const float* __restrict__ orig0, const float* __restrict__ orig1,
                                                               float* __restrict__ pack15, int pack_ld, _Float16* __restrict__ pack_hi,
                                                               _Float16* __restrict__ pack_lo, long long pack_rows, int pack_c0, int B, int H,
                                                               int W) {
    fp16_saturate_on();
    __shared__ __attribute__((aligned(16))) float tile[2][3 * WB_PLANE];
    __shared__ int bx[2][4];
    const int tid = threadIdx.x;
    const long long hw = (long long)H * W;
    int b, x, y;
    bool live;
    tile_pixel(H, W, b, x, y, live);
    const long long pix = (long long)(live ? y : 0) * W + (live ? x : 0);
    if (tid < 2) box_reset(bx[tid]);
    const float* mp = motion + b * motion_bstride + pix * motion_ld;
    const float fx0 = mp[0], fy0 = mp[1], fx1 = mp[2], fy1 = mp[3];
    const float m1 = sigmoidf_(mp[4]);
    const float m2 = 1.0f - m1;
    const Taps t0 = make_taps((float)x + fx0, (float)y + fy0, W, H);
    const Taps t1 = make_taps((float)x + fx1, (float)y + fy1, W, H);
    __syncthreads();
    box_add(bx[0], t0, live, W, H);
    box_add(bx[1], t1, live, W, H);
    __syncthreads();
    const StagedBox s0 = box_get(bx[0]), s1 = box_get(bx[1]);
    if (s0.ok) box_stage(tile[0], im0 + (long long)b * 3 * hw, hw, W, 3, s0, tid);
    if (s1.ok) box_stage(tile[1], im1 + (long long)b * 3 * hw, hw, W, 3, s1, tid);
    __syncthreads();
    if (!live) return;
    float a[3], c[3], o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const long long pl = ((long long)b * 3 + ch) * hw;
        a[ch] = s0.ok ? sample_tile(tile[0] + ch * WB_PLANE, t0, s0) : sample_plane(im0 + pl, t0, W);
        c[ch] = s1.ok ? sample_tile(tile[1] + ch * WB_PLANE, t1, s1) : sample_plane(im1 + pl, t1, W);
        o[ch] = m1 * a[ch] + m2 * c[ch];
        i0w[pl + pix] = a[ch];
        i1w[pl + pix] = c[ch];
        it[pl + pix] = o[ch];
    }
    if (f0o) {
        f0o[((long long)b * 2) * hw + pix] = fx0;
        f0o[((long long)b * 2 + 1) * hw + pix] = fy0;
        f1o[((long long)b * 2) * hw + pix] = fx1;
        f1o[((long long)b * 2 + 1) * hw + pix] = fy1;
    }
    if (m1o) {
        m1o[(long long)b * hw + pix] = m1;
        m2o[(long long)b * hw + pix] = m2;
    }
    if (pack15) {
        float* pp = pack15 + ((long long)b * hw + pix) * pack_ld;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long pl = ((long long)b * 3 + ch) * hw + pix;
            pp[ch] = orig0[pl];
            pp[3 + ch] = a[ch];
            pp[6 + ch] = orig1[pl];
            pp[9 + ch] = c[ch];
            pp[12 + ch] = o[ch];
        }
    }
    if (pack_hi) {
        float v16[16];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long pl = ((long long)b * 3 + ch) * hw + pix;
            v16[ch] = orig0[pl];
            v16[3 + ch] = a[ch];
            v16[6 + ch] = orig1[pl];
            v16[9 + ch] = c[ch];
            v16[12 + ch] = o[ch];
        }
        v16[15] = 0.f;
        const RowSink sink{nullptr, 0, pack_hi, pack_lo, pack_rows};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            sink_store4(sink, (long long)b * hw + pix, pack_c0 + 4 * q, (f32x4){v16[4 * q], v16[4 * q + 1], v16[4 * q + 2], v16[4 * q + 3]});
    }
}

// ---------------------------------------------------------------------------------------
// align_corners=True bilinear resize, planar, any source strides
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resize_ac_kernel(const float* __restrict__ src, long long sb, long long sc, long long sy,
                                                        long long sx, float* __restrict__ dst, int B, int C,
                                                        int Hi, int Wi, int Ho, int Wo, float value_scale) {
    fp16_saturate_on();
    const float sh = ac_scale(Hi, Ho), sw = ac_scale(Wi, Wo);
    const long long ohw = (long long)Ho * Wo;
    const long long total = (long long)B * C * ohw;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(idx / ohw);
        const int pb = p / C, pc = p - pb * C;
        const long long pix = idx - (long long)p * ohw;
        const int oy = (int)(pix / Wo), ox = (int)(pix - (long long)oy * Wo);
        const AcTaps a = ac_taps(sh, sw, oy, ox, Hi, Wi);
        const float* s = src + pb * sb + pc * sc + a.y0 * sy + a.x0 * sx;
        const float v = ac_blend(a, s[0], s[a.xp * sx], s[a.yp * sy], s[a.yp * sy + a.xp * sx]);
        dst[idx] = v * value_scale;
    }
}

// element e of torch.cat([im0, im1], 0) as NHWC4 (the encoder's input): stacked frame [im0 batch..., im1 batch...], pixel, 3 channels + 0
__device__ __forceinline__ void pack_frame_element(const float* __restrict__ im0, const float* __restrict__ im1, float* __restrict__ dst,
                                                   long long e, int B, long long hw) {
    const int f = (int)(e / hw);
    const long long pix = e - (long long)f * hw;
    const float* s = (f < B ? im0 + (long long)f * 3 * hw : im1 + (long long)(f - B) * 3 * hw) + pix;
    *reinterpret_cast<f32x4*>(dst + e * 4) = (f32x4){s[0], s[hw], s[2 * hw], 0.f};
}

// The three x0.5 image-pyramid levels of both frames in ONE launch (network_base.py:444-448: F.interpolate(scale 0.5, bilinear,
// align_corners=True) applied level by level).  A thread owns one output element of one level and evaluates the levels below it on
// the fly with the resize's arithmetic, in its order -- bit-identical to three sequential resizes (level 3 costs 64 reads
// of the frame per element; it has 1 / 64 of the frame's pixels).  Four dependent 7-us launches become one.
template <int L>
__device__ __forceinline__ float pyramid_value(const float* __restrict__ plane, int H, int W, int oy, int ox) {
    if constexpr (L == 0) {
        return plane[(long long)oy * W + ox];
    } else {
        const int Hi = H >> (L - 1), Wi = W >> (L - 1);
        const AcTaps a = ac_taps(ac_scale(Hi, H >> L), ac_scale(Wi, W >> L), oy, ox, Hi, Wi);
        const float v00 = pyramid_value<L - 1>(plane, H, W, a.y0, a.x0), v01 = pyramid_value<L - 1>(plane, H, W, a.y0, a.x0 + a.xp);
        const float v10 = pyramid_value<L - 1>(plane, H, W, a.y0 + a.yp, a.x0), v11 = pyramid_value<L - 1>(plane, H, W, a.y0 + a.yp, a.x0 + a.xp);
        const float v = ac_blend(a, v00, v01, v10, v11);
        return v * 1.0f;
    }
}

__global__ __launch_bounds__(256) void image_pyramid_kernel(const float* __restrict__ im0, const float* __restrict__ im1, float* __restrict__ l1,
                                                            float* __restrict__ l2, float* __restrict__ l3, float* __restrict__ pack, int B, int H, int W) {
    fp16_saturate_on();
    const long long n1 = (long long)(H >> 1) * (W >> 1), n2 = (long long)(H >> 2) * (W >> 2), n3 = (long long)(H >> 3) * (W >> 3);
    const long long planes = 2ll * B * 3;
    const long long t1 = planes * n1, t2 = planes * n2, t3 = planes * n3;
    const long long hw = (long long)H * W, tp = pack ? 2ll * B * hw : 0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < t1 + t2 + t3 + tp; idx += (long long)gridDim.x * blockDim.x) {
        if (idx >= t1 + t2 + t3) {      // pack_frames' work in the same launch
            pack_frame_element(im0, im1, pack, idx - (t1 + t2 + t3), B, hw);
            continue;
        }
        const int lvl = idx < t1 ? 1 : (idx < t1 + t2 ? 2 : 3);
        const long long e = idx - (lvl == 1 ? 0 : (lvl == 2 ? t1 : t1 + t2));
        const long long n = lvl == 1 ? n1 : (lvl == 2 ? n2 : n3);
        const int pl = (int)(e / n);                                   // stacked plane: [im0 batch x 3, im1 batch x 3]
        const long long pix = e - (long long)pl * n;
        const int Wo = W >> lvl;
        const int oy = (int)(pix / Wo), ox = (int)(pix - (long long)oy * Wo);
        const float* src = (pl < 3 * B ? im0 + (long long)pl * H * W : im1 + (long long)(pl - 3 * B) * H * W);
        if (lvl == 1) l1[e] = pyramid_value<1>(src, H, W, oy, ox);
        else if (lvl == 2) l2[e] = pyramid_value<2>(src, H, W, oy, ox);
        else l3[e] = pyramid_value<3>(src, H, W, oy, ox);
    }
}

__global__ __launch_bounds__(256) void pack_frames_kernel(const float* __restrict__ im0, const float* __restrict__ im1,
                                                          float* __restrict__ dst, int B, int H, int W) {
    fp16_saturate_on();
    const long long hw = (long long)H * W;
    const long long total = 2ll * B * hw;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x)
        pack_frame_element(im0, im1, dst, idx, B, hw);
}

// ---------------------------------------------------------------------------------------
// Half-resolution motion (include/atmvfi.h, ABI 0.26; atm-vfi_amd/scaled.py holds the definition and the numpy twins).
// frame_half: the 2 x 2 box average ((a + b) + (c + d)) * 0.25f.  VEC: a lane owns four adjacent outputs of a row (two 16-byte loads per
// source row, one 16-byte store); else one output, scalar accesses.  The same expression per output: the same bits.
// ---------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void frame_half_kernel(const float* __restrict__ src, float* __restrict__ dst, long long rows, int w) {
    fp16_saturate_on();
    const int W = 2 * w;
    if constexpr (VEC) {
        const int wv = w >> 2;                                   // W % 8 == 0
        const long long total = rows * wv;                       // rows: planes * h output rows; output row r reads source rows 2r, 2r + 1
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const long long r = idx / wv;
            const int v = (int)(idx - r * wv);
            const float* s = src + 2 * r * W + 8 * v;
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(s), t1 = *reinterpret_cast<const f32x4*>(s + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(s + W), b1 = *reinterpret_cast<const f32x4*>(s + W + 4);
            f32x4 o;
            o.x = ((t0.x + t0.y) + (b0.x + b0.y)) * 0.25f;
            o.y = ((t0.z + t0.w) + (b0.z + b0.w)) * 0.25f;
            o.z = ((t1.x + t1.y) + (b1.x + b1.y)) * 0.25f;
            o.w = ((t1.z + t1.w) + (b1.z + b1.w)) * 0.25f;
            *reinterpret_cast<f32x4*>(dst + r * w + 4 * v) = o;
        }
    } else {
        const long long total = rows * w;
        for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
            const long long r = idx / w;
            const int x = (int)(idx - r * w);
            const float* s = src + 2 * r * W + 2 * x;
            dst[idx] = ((s[0] + s[1]) + (s[W] + s[W + 1])) * 0.25f;
        }
    }
}

// synth_up2: full-size synthesis from a half-size forward.  The workgroup's 32 x 8 output tile (tile_pixel) reads the half-size pixels
// of columns X0/2 - 1 .. X0/2 + 16 and rows Y0/2 - 1 .. Y0/2 + 4: lanes 0 .. 107 build them in LDS as eight interleaved floats
// f0x f0y f1x f1y | m rR rG rB (r: the residual it_sum - blend, warp_blend's expression), every lane blends its four with the 0.25 / 0.75
// rule, and from there on the kernel is warp_blend_tiled_kernel's: taps, boxes, staged or gathered samples.  The half-size pixels live in
// the first 3.4 KiB of source box 0, which is staged only after the barrier that follows their last read.  STAGED = false: gathers throughout
// (any width and alignment; the default: it measured faster); the arithmetic is shared, so the two instances give the same bits.
// Tried and dropped, both slower at 2176 x 4096 (README, "Half-resolution motion"): a half-size pre-pass that interleaves the eight maps
// into a workspace (it moves more bytes than the 1.7-fold re-reading it saves), and a lane per 2 x 2 output quad on that pre-pass.
struct SynthUp2Args {
    const float *it_sum, *it0, *it1, *flow0, *flow1, *m1, *store0, *store1;
    float *dst, *f0o, *f1o, *mo;
    unsigned char* dst_u8;
    int h, w, pad_top, pad_left, hh, ww, bgr;
    int s0[16], s1[16];
};
constexpr int UP_W = WT_W / 2 + 2, UP_H = WT_H / 2 + 2;       // half-size neighbourhood of an output tile
static_assert(UP_W * UP_H <= 256 && UP_W * UP_H * 8 <= 3 * WB_PLANE, "the neighbourhood is built by one pass of the workgroup inside box 0");

__device__ __forceinline__ f32x4 up2_blend(float wy0, float wy1, float wx0, float wx1, f32x4 v00, f32x4 v01, f32x4 v10, f32x4 v11) {
    return wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
}

// sample_plane with its four loads issued unconditionally: a tap outside the image reads the nearest pixel inside and is dropped by a
// select, so the sum is sample_plane's, bit for bit, for any source values.  sample_plane's `if (in) v += ...` compiles to one masked
// block per tap with a wait in each; over two sources and three planes that was a chain of dependent memory latencies (counter passes on
// the MI355X: 88 % of the direct instance's wave cycles were waits while HBM ran at 27 %); here the 24 loads of a pixel are in flight together.
__device__ __forceinline__ float sample_plane_all(const float* __restrict__ p, const Taps& t, int W, int H) {
    const int xa = t.x0 < 0 ? 0 : (t.x0 > W - 1 ? W - 1 : t.x0), xb = t.x0 + 1 < 0 ? 0 : (t.x0 + 1 > W - 1 ? W - 1 : t.x0 + 1);
    const int ya = t.y0 < 0 ? 0 : (t.y0 > H - 1 ? H - 1 : t.y0), yb = t.y0 + 1 < 0 ? 0 : (t.y0 + 1 > H - 1 ? H - 1 : t.y0 + 1);
    const float* ra = p + (long long)ya * W;
    const float* rb = p + (long long)yb * W;
    const float b00 = ra[xa], b01 = ra[xb], b10 = rb[xa], b11 = rb[xb];
    float v = 0.f;                                        // (each sum is formed, then selected: a conditional sum would pull its load into a branch)
    const float v0 = v + b00 * t.w00;
    v = t.in00 ? v0 : v;
    const float v1 = v + b01 * t.w01;
    v = t.in01 ? v1 : v;
    const float v2 = v + b10 * t.w10;
    v = t.in10 ? v2 : v;
    const float v3 = v + b11 * t.w11;
    v = t.in11 ? v3 : v;
    return v;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void synth_up2_kernel(const SynthUp2Args p) {
    fp16_saturate_on();
    __shared__ __attribute__((aligned(16))) float lds[STAGED ? 2 * 3 * WB_PLANE : UP_W * UP_H * 8];
    __shared__ int bx[2][4];
    float* const tile[2] = {lds, lds + (STAGED ? 3 * WB_PLANE : 0)};
    const int tid = threadIdx.x;
    const int H = 2 * p.h, W = 2 * p.w;
    const long long hw = (long long)H * W, qhw = (long long)p.h * p.w;
    int b, x, y;
    bool live;
    tile_pixel(H, W, b, x, y, live);
    const int ox = ((x - (tid & (WT_W - 1))) >> 1) - 1, oy = ((y - (tid >> 5)) >> 1) - 1;      // half-size origin of the neighbourhood
    float* up = tile[0];
    if (tid < 2) box_reset(bx[tid]);
    if (tid < UP_W * UP_H) {
        const int r = tid / UP_W, qy = oy + r, qx = ox + (tid - r * UP_W);
        if (qx >= 0 && qx < p.w && qy >= 0 && qy < p.h) {
            const long long q = (long long)qy * p.w + qx;
            const float* f0 = p.flow0 + (long long)b * 2 * qhw + q;
            const float* f1 = p.flow1 + (long long)b * 2 * qhw + q;
            const float m1 = p.m1[(long long)b * qhw + q];
            float res[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const long long o = ((long long)b * 3 + ch) * qhw + q;
                res[ch] = p.it_sum[o] - (m1 * p.it0[o] + (1.0f - m1) * p.it1[o]);
            }
            *reinterpret_cast<f32x4*>(up + tid * 8) = (f32x4){f0[0], f0[qhw], f1[0], f1[qhw]};
            *reinterpret_cast<f32x4*>(up + tid * 8 + 4) = (f32x4){m1, res[0], res[1], res[2]};
        }
    }
    __syncthreads();
    // the four half-size pixels of this output (a lane outside the image takes the last row / column's: it only has to stay in the LDS block)
    const int xc = x < W ? x : W - 1, yc = y < H ? y : H - 1;
    const bool xodd = xc & 1, yodd = yc & 1;
    const int c0 = xodd ? (xc - 1) >> 1 : ((xc >> 1) - 1 < 0 ? 0 : (xc >> 1) - 1), c1 = xodd ? (((xc + 1) >> 1) > p.w - 1 ? p.w - 1 : (xc + 1) >> 1) : xc >> 1;
    const int r0 = yodd ? (yc - 1) >> 1 : ((yc >> 1) - 1 < 0 ? 0 : (yc >> 1) - 1), r1 = yodd ? (((yc + 1) >> 1) > p.h - 1 ? p.h - 1 : (yc + 1) >> 1) : yc >> 1;
    const float wx0 = xodd ? 0.75f : 0.25f, wx1 = xodd ? 0.25f : 0.75f, wy0 = yodd ? 0.75f : 0.25f, wy1 = yodd ? 0.25f : 0.75f;
    const float* u00 = up + ((r0 - oy) * UP_W + (c0 - ox)) * 8;
    const float* u01 = up + ((r0 - oy) * UP_W + (c1 - ox)) * 8;
    const float* u10 = up + ((r1 - oy) * UP_W + (c0 - ox)) * 8;
    const float* u11 = up + ((r1 - oy) * UP_W + (c1 - ox)) * 8;
    const f32x4 fl = up2_blend(wy0, wy1, wx0, wx1, *reinterpret_cast<const f32x4*>(u00), *reinterpret_cast<const f32x4*>(u01),
                               *reinterpret_cast<const f32x4*>(u10), *reinterpret_cast<const f32x4*>(u11));
    const f32x4 mr = up2_blend(wy0, wy1, wx0, wx1, *reinterpret_cast<const f32x4*>(u00 + 4), *reinterpret_cast<const f32x4*>(u01 + 4),
                               *reinterpret_cast<const f32x4*>(u10 + 4), *reinterpret_cast<const f32x4*>(u11 + 4));
    const float fx0 = fl.x * 2.0f, fy0 = fl.y * 2.0f, fx1 = fl.z * 2.0f, fy1 = fl.w * 2.0f;
    const float m = mr.x;
    const Taps t0 = make_taps((float)x + fx0, (float)y + fy0, W, H);
    const Taps t1 = make_taps((float)x + fx1, (float)y + fy1, W, H);
    const float* im0 = p.store0 + (long long)p.s0[b] * 3 * hw;
    const float* im1 = p.store1 + (long long)p.s1[b] * 3 * hw;
    StagedBox s0, s1;
    s0.ok = s1.ok = false;
    if constexpr (STAGED) {
        box_add(bx[0], t0, live, W, H);
        box_add(bx[1], t1, live, W, H);
        __syncthreads();                                  // also: every lane has read its half-size pixels, box 0 may be overwritten
        s0 = box_get(bx[0]);
        s1 = box_get(bx[1]);
        if (s0.ok) box_stage(tile[0], im0, hw, W, 3, s0, tid);
        if (s1.ok) box_stage(tile[1], im1, hw, W, 3, s1, tid);
        __syncthreads();
    }
    if (!live) return;
    const long long pix = (long long)y * W + x;
    const int wy = y - p.pad_top, wx = x - p.pad_left;
    const bool in_window = p.dst_u8 && wy >= 0 && wy < p.hh && wx >= 0 && wx < p.ww;
    int q8[3];
    float a3[3], c3[3];                                   // every sample before the first store: an output may alias nothing, but the
#pragma unroll                                            // compiler cannot know, and a store between would split the loads again
    for (int ch = 0; ch < 3; ++ch) {
        a3[ch] = s0.ok ? sample_tile(tile[0] + ch * WB_PLANE, t0, s0) : sample_plane_all(im0 + ch * hw, t0, W, H);
        c3[ch] = s1.ok ? sample_tile(tile[1] + ch * WB_PLANE, t1, s1) : sample_plane_all(im1 + ch * hw, t1, W, H);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a = a3[ch], c = c3[ch];
        const float res = ch == 0 ? mr.y : (ch == 1 ? mr.z : mr.w);
        const float v = fminf(fmaxf((m * a + (1.0f - m) * c) + res, 0.0f), 1.0f);
        if (p.dst) p.dst[((long long)b * 3 + ch) * hw + pix] = v;
        const int q = __float2int_rn(v * 255.0f);        // rint: half to even, as np.round (frame_f32_to_u8)
        q8[ch] = q < 0 ? 0 : (q > 255 ? 255 : q);
    }
    if (in_window) {
        unsigned char* o = p.dst_u8 + (((long long)b * p.hh + wy) * p.ww + wx) * 3;
        o[0] = (unsigned char)(p.bgr ? q8[2] : q8[0]);
        o[1] = (unsigned char)q8[1];
        o[2] = (unsigned char)(p.bgr ? q8[0] : q8[2]);
    }
    if (p.f0o) {
        p.f0o[((long long)b * 2) * hw + pix] = fx0;
        p.f0o[((long long)b * 2 + 1) * hw + pix] = fy0;
        p.f1o[((long long)b * 2) * hw + pix] = fx1;
        p.f1o[((long long)b * 2 + 1) * hw + pix] = fy1;
    }
    if (p.mo) p.mo[(long long)b * hw + pix] = m;
}

// ---------------------------------------------------------------------------------------
// Launchers.  Checks that several entry points share are made once, under the caller's name `who`.
// ---------------------------------------------------------------------------------------
long long warp_tiles(int B, int H, int W) { return (long long)B * ((H + WT_H - 1) / WT_H) * ((W + WT_W - 1) / WT_W); }

// flow_warp, _ex, _tiled, _up2, _up2_tiled: pointers (ptrs: all of them non-null), shape, and for the tiled forms the 16-byte rows
int check_warp(const char* who, bool ptrs, bool tiled, const float* src, int B, int C, int H, int W) {
    ATMVFI_REQUIRE(ptrs, ATMVFI_EINVAL, "%s: null pointer", who);
    ATMVFI_REQUIRE(B > 0 && C > 0 && H > 1 && W > 1, ATMVFI_EINVAL, "%s: bad shape (H, W must be > 1)", who);
    if (tiled)
        ATMVFI_REQUIRE(W % 4 == 0 && atmvfi::aligned16(src), ATMVFI_EINVAL, "%s: W must be a multiple of 4 and src 16-byte aligned (got W = %d)", who, W);
    return ATMVFI_OK;
}

int check_blend(const char* who, bool tiled, const float* im0, const float* im1, const float* motion, int motion_ld, const float* i0w,
                const float* i1w, const float* it, const float* flow0_out, const float* flow1_out, const float* mask1_out,
                const float* mask2_out, const float* orig0, const float* orig1, const float* pack15, int pack_ld, const void* pack_hi,
                const void* pack_lo, int64_t pack_rows, int pack_c0, int B, int H, int W) {
    ATMVFI_REQUIRE(im0 && im1 && motion && i0w && i1w && it, ATMVFI_EINVAL, "%s: null pointer", who);
    ATMVFI_REQUIRE(B > 0 && H > 1 && W > 1 && motion_ld >= 5, ATMVFI_EINVAL, "%s: bad shape", who);
    if (tiled)
        ATMVFI_REQUIRE(W % 4 == 0 && atmvfi::aligned16(im0) && atmvfi::aligned16(im1), ATMVFI_EINVAL,
                       "%s: W must be a multiple of 4 and the images 16-byte aligned (got W = %d)", who, W);
    ATMVFI_REQUIRE((flow0_out == nullptr) == (flow1_out == nullptr) && (mask1_out == nullptr) == (mask2_out == nullptr),
                   ATMVFI_EINVAL, "%s: flow/mask outputs come in pairs", who);
    if (pack15) ATMVFI_REQUIRE(orig0 && orig1 && pack_ld >= 15, ATMVFI_EINVAL, "%s: pack15 needs orig0/orig1 and ld >= 15", who);
    ATMVFI_REQUIRE((pack_hi == nullptr) == (pack_lo == nullptr), ATMVFI_EINVAL, "%s: the plane sink needs both planes", who);
    if (pack_hi)
        ATMVFI_REQUIRE(orig0 && orig1 && pack_rows >= (int64_t)B * H * W && pack_c0 >= 0 && pack_c0 % 4 == 0 && atmvfi::aligned16(pack_hi) &&
                           atmvfi::aligned16(pack_lo), ATMVFI_EINVAL,
                       "%s: plane sink needs orig0/orig1, rows >= B*H*W, a channel offset that is a multiple of 4, aligned planes", who);
    if (tiled) ATMVFI_REQUIRE(warp_tiles(B, H, W) < (1ll << 31), ATMVFI_EINVAL, "%s: grid too large", who);
    return ATMVFI_OK;
}

// the one host path of atmvfi_warp_blend, _planes (both report as warp_blend) and _tiled
int launch_blend(const char* who, bool tiled, const float* im0, const float* im1, const float* motion, int motion_ld, int64_t motion_bstride,
                 float* i0w, float* i1w, float* it, float* flow0_out, float* flow1_out, float* mask1_out, float* mask2_out, const float* orig0,
                 const float* orig1, float* pack15, int pack_ld, void* pack_hi, void* pack_lo, int64_t pack_rows, int pack_c0, int B, int H, int W,
                 void* stream) {
    if (const int rc = check_blend(who, tiled, im0, im1, motion, motion_ld, i0w, i1w, it, flow0_out, flow1_out, mask1_out, mask2_out, orig0, orig1,
                                   pack15, pack_ld, pack_hi, pack_lo, pack_rows, pack_c0, B, H, W))
        return rc;
    const unsigned blocks = tiled ? (unsigned)warp_tiles(B, H, W) : grid_for((long long)B * H * W);
    hipLaunchKernelGGL((tiled ? warp_blend_tiled_kernel : warp_blend_kernel), dim3(blocks), dim3(256), 0, (hipStream_t)stream, im0, im1, motion,
                       motion_ld, (long long)motion_bstride, i0w, i1w, it, flow0_out, flow1_out, mask1_out, mask2_out, orig0, orig1, pack15,
                       pack_ld, (_Float16*)pack_hi, (_Float16*)pack_lo, (long long)pack_rows, pack_c0, B, H, W);
    return atmvfi::check_launch(who);
}

}  // namespace

extern "C" int atmvfi_flow_warp(const float* src, const float* flow, int64_t flow_bstride, int flow_pstride,
                                 int flow_cstride, float* dst, int B, int C, int H, int W, void* stream) {
    if (const int rc = check_warp("flow_warp", src && flow && dst, false, src, B, C, H, W)) return rc;
    hipLaunchKernelGGL(flow_warp_planar_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, src,
                       flow, (long long)flow_bstride, flow_pstride, flow_cstride, dst, B, C, H, W);
    return atmvfi::check_launch("flow_warp");
}

extern "C" int atmvfi_flow_warp_ex(const float* src, const float* flow, float* dst, uint8_t* mask, int B, int C, int H, int W,
                                    int padding_mode, void* stream) {
    if (const int rc = check_warp("flow_warp_ex", src && flow && dst, false, src, B, C, H, W)) return rc;
    ATMVFI_REQUIRE(padding_mode >= 0 && padding_mode <= 2, ATMVFI_EINVAL, "flow_warp_ex: padding_mode must be 0 (zeros), 1 (border) or 2 (reflection), got %d", padding_mode);
    hipLaunchKernelGGL(flow_warp_ex_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, src, flow, dst,
                       (unsigned char*)mask, B, C, H, W, padding_mode);
    return atmvfi::check_launch("flow_warp_ex");
}

extern "C" int atmvfi_flow_warp_tiled(const float* src, const float* flow, int64_t flow_bstride, int flow_pstride,
                                       int flow_cstride, float* dst, int B, int C, int H, int W, void* stream) {
    if (const int rc = check_warp("flow_warp_tiled", src && flow && dst, true, src, B, C, H, W)) return rc;
    const long long tiles = warp_tiles(B, H, W);
    ATMVFI_REQUIRE(tiles < (1ll << 31), ATMVFI_EINVAL, "flow_warp_tiled: grid too large");
    hipLaunchKernelGGL(flow_warp_tiled_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, src, flow, (long long)flow_bstride,
                       flow_pstride, flow_cstride, dst, B, C, H, W);
    return atmvfi::check_launch("flow_warp_tiled");
}

extern "C" int atmvfi_flow_warp_up2(const float* src, const float* flow, float* dst, float* flow_up, int B, int C, int H, int W, void* stream) {
    if (const int rc = check_warp("flow_warp_up2", src && flow && dst && flow_up, false, src, B, C, H, W)) return rc;
    hipLaunchKernelGGL(flow_warp_up2_kernel, dim3(grid_for((long long)B * H * W * 9)), dim3(256), 0, (hipStream_t)stream, src, flow, dst, flow_up,
                       B, C, H, W);
    return atmvfi::check_launch("flow_warp_up2");
}

extern "C" int atmvfi_flow_warp_up2_tiled(const float* src, const float* flow, float* dst, float* flow_up, int B, int C, int H, int W, void* stream) {
    if (const int rc = check_warp("flow_warp_up2_tiled", src && flow && dst && flow_up, true, src, B, C, H, W)) return rc;
    const long long tiles = warp_tiles(B, H, W);
    const long long upblocks = grid_for((long long)B * H * W * 8);
    ATMVFI_REQUIRE(tiles + upblocks < (1ll << 31), ATMVFI_EINVAL, "flow_warp_up2_tiled: grid too large");
    hipLaunchKernelGGL(flow_warp_up2_tiled_kernel, dim3((unsigned)(tiles + upblocks)), dim3(256), 0, (hipStream_t)stream, src, flow, dst, flow_up,
                       B, C, H, W, (int)tiles);
    return atmvfi::check_launch("flow_warp_up2_tiled");
}

extern "C" int atmvfi_flow_warp_nhwc(const float* src, int src_ld, int64_t src_bstride, const float* flow,
                                      int64_t flow_bstride, int flow_pstride, int flow_cstride, float* dst, int dst_ld,
                                      int64_t dst_bstride, int B, int C, int H, int W, void* stream) {
    ATMVFI_REQUIRE(src && flow && dst, ATMVFI_EINVAL, "flow_warp_nhwc: null pointer");
    ATMVFI_REQUIRE(B > 0 && C > 0 && C % 4 == 0 && H > 1 && W > 1, ATMVFI_EINVAL, "flow_warp_nhwc: bad shape");
    ATMVFI_REQUIRE(src_ld % 4 == 0 && dst_ld % 4 == 0 && src_bstride % 4 == 0 && dst_bstride % 4 == 0 &&
                       atmvfi::aligned16(src) && atmvfi::aligned16(dst),
                   ATMVFI_EALIGN, "flow_warp_nhwc: views must be 16-byte aligned");
    hipLaunchKernelGGL(flow_warp_nhwc_kernel, dim3(grid_for((long long)B * H * W * (C / 4))), dim3(256), 0,
                       (hipStream_t)stream, src, src_ld, (long long)src_bstride, flow, (long long)flow_bstride, flow_pstride,
                       flow_cstride, dst, dst_ld, (long long)dst_bstride, B, C, H, W);
    return atmvfi::check_launch("flow_warp_nhwc");
}

extern "C" int atmvfi_warp_blend_planes(const float* im0, const float* im1, const float* motion, int motion_ld,
                                         int64_t motion_bstride, float* i0w, float* i1w, float* it, float* flow0_out,
                                         float* flow1_out, float* mask1_out, float* mask2_out, const float* orig0,
                                         const float* orig1, float* pack15, int pack_ld, void* pack_hi, void* pack_lo, int64_t pack_rows,
                                         int pack_c0, int B, int H, int W, void* stream) {
    return launch_blend("warp_blend", false, im0, im1, motion, motion_ld, motion_bstride, i0w, i1w, it, flow0_out, flow1_out, mask1_out, mask2_out,
                        orig0, orig1, pack15, pack_ld, pack_hi, pack_lo, pack_rows, pack_c0, B, H, W, stream);
}
extern "C" int atmvfi_warp_blend_tiled(const float* im0, const float* im1, const float* motion, int motion_ld,
                                        int64_t motion_bstride, float* i0w, float* i1w, float* it, float* flow0_out,
                                        float* flow1_out, float* mask1_out, float* mask2_out, const float* orig0,
                                        const float* orig1, float* pack15, int pack_ld, void* pack_hi, void* pack_lo, int64_t pack_rows,
                                        int pack_c0, int B, int H, int W, void* stream) {
    return launch_blend("warp_blend_tiled", true, im0, im1, motion, motion_ld, motion_bstride, i0w, i1w, it, flow0_out, flow1_out, mask1_out,
                        mask2_out, orig0, orig1, pack15, pack_ld, pack_hi, pack_lo, pack_rows, pack_c0, B, H, W, stream);
}
extern "C" int atmvfi_warp_blend(const float* im0, const float* im1, const float* motion, int motion_ld,
                                  int64_t motion_bstride, float* i0w, float* i1w, float* it, float* flow0_out,
                                  float* flow1_out, float* mask1_out, float* mask2_out, const float* orig0,
                                  const float* orig1, float* pack15, int pack_ld, int B, int H, int W, void* stream) {
    return launch_blend("warp_blend", false, im0, im1, motion, motion_ld, motion_bstride, i0w, i1w, it, flow0_out, flow1_out, mask1_out, mask2_out,
                        orig0, orig1, pack15, pack_ld, nullptr, nullptr, 0, 0, B, H, W, stream);
}

extern "C" int atmvfi_resize_bilinear_ac(const float* src, int64_t src_bstride, int64_t src_cstride, int64_t src_ystride,
                                          int64_t src_xstride, float* dst, int B, int C, int Hi, int Wi, int Ho, int Wo,
                                          float value_scale, void* stream) {
    ATMVFI_REQUIRE(src && dst, ATMVFI_EINVAL, "resize_bilinear_ac: null pointer");
    ATMVFI_REQUIRE(B > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, ATMVFI_EINVAL, "resize_bilinear_ac: bad shape");
    hipLaunchKernelGGL(resize_ac_kernel, dim3(grid_for((long long)B * C * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, src,
                       (long long)src_bstride, (long long)src_cstride, (long long)src_ystride, (long long)src_xstride, dst,
                       B, C, Hi, Wi, Ho, Wo, value_scale);
    return atmvfi::check_launch("resize_bilinear_ac");
}

extern "C" int atmvfi_image_pyramid_pack(const float* im0, const float* im1, float* l1, float* l2, float* l3, float* pack, int B, int H, int W,
                                         void* stream) {
    ATMVFI_REQUIRE(im0 && im1 && l1 && l2 && l3, ATMVFI_EINVAL, "image_pyramid: null pointer");
    // any size with a non-empty level 3: the kernel takes level l as (H >> l) x (W >> l), F.interpolate(scale_factor=0.5)'s floor
    ATMVFI_REQUIRE(B > 0 && H >= 8 && W >= 8, ATMVFI_EINVAL, "image_pyramid: H, W must be at least 8 (got %dx%d)", H, W);
    ATMVFI_REQUIRE(!pack || atmvfi::aligned16(pack), ATMVFI_EALIGN, "image_pyramid: pack must be 16-byte aligned");
    const long long total = 2ll * B * 3 * ((long long)(H >> 1) * (W >> 1) + (long long)(H >> 2) * (W >> 2) + (long long)(H >> 3) * (W >> 3)) +
                            (pack ? 2ll * B * H * W : 0);
    hipLaunchKernelGGL(image_pyramid_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, im0, im1, l1, l2, l3, pack, B, H, W);
    return atmvfi::check_launch("image_pyramid");
}

extern "C" int atmvfi_image_pyramid(const float* im0, const float* im1, float* l1, float* l2, float* l3, int B, int H, int W, void* stream) {
    return atmvfi_image_pyramid_pack(im0, im1, l1, l2, l3, nullptr, B, H, W, stream);
}

extern "C" int atmvfi_pack_frames(const float* im0, const float* im1, float* dst, int B, int H, int W, void* stream) {
    ATMVFI_REQUIRE(im0 && im1 && dst && B > 0 && H > 0 && W > 0, ATMVFI_EINVAL, "pack_frames: bad arguments");
    ATMVFI_REQUIRE(atmvfi::aligned16(dst), ATMVFI_EALIGN, "pack_frames: dst must be 16-byte aligned");
    hipLaunchKernelGGL(pack_frames_kernel, dim3(grid_for(2ll * B * H * W)), dim3(256), 0, (hipStream_t)stream, im0, im1, dst,
                       B, H, W);
    return atmvfi::check_launch("pack_frames");
}

// ---------------------------------------------------------------------------------------
// Half-resolution motion: host checks and launches
// ---------------------------------------------------------------------------------------
namespace {
struct ByteRange {
    const void* p;
    long long n;
    const char* name;
};
bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p && b.p && a.n > 0 && b.n > 0 && a0 < b0 + (uintptr_t)b.n && b0 < a0 + (uintptr_t)a.n;
}
bool synth_up2_shape_ok(long long B, long long h, long long w) { return B >= 1 && B <= 16 && h >= 1 && w >= 1 && h < (1 << 24) && w < (1 << 24); }
}  // namespace

extern "C" int atmvfi_frame_half(const float* src, float* dst, int planes, int H, int W, void* stream) {
    ATMVFI_REQUIRE(src && dst, ATMVFI_EINVAL, "frame_half: null pointer");
    ATMVFI_REQUIRE(planes >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, ATMVFI_EINVAL,
                   "frame_half: planes must be positive and H, W even and at least 2 (got %d planes of %d x %d)", planes, H, W);
    const long long n = (long long)planes * H * W;
    ATMVFI_REQUIRE(!ranges_overlap({src, n * 4, "src"}, {dst, n, "dst"}), ATMVFI_EINVAL, "frame_half: src and dst overlap");
    const long long rows = (long long)planes * (H / 2);
    const int w = W / 2;
    if (W % 8 == 0 && atmvfi::aligned16(src) && atmvfi::aligned16(dst))
        hipLaunchKernelGGL(frame_half_kernel<true>, dim3(grid_for(rows * (w / 4))), dim3(256), 0, (hipStream_t)stream, src, dst, rows, w);
    else
        hipLaunchKernelGGL(frame_half_kernel<false>, dim3(grid_for(rows * w)), dim3(256), 0, (hipStream_t)stream, src, dst, rows, w);
    return atmvfi::check_launch("frame_half");
}

extern "C" int64_t atmvfi_synth_up2_workspace_floats(int B, int h, int w) { return synth_up2_shape_ok(B, h, w) ? 0 : -1; }

extern "C" int atmvfi_synth_up2(const atmvfi_synth_up2_params* p, void* stream) {
    ATMVFI_REQUIRE(p, ATMVFI_EINVAL, "synth_up2: null parameter block");
    ATMVFI_REQUIRE(p->it_sum && p->it0 && p->it1 && p->flow0 && p->flow1 && p->m1 && p->store0 && p->store1, ATMVFI_EINVAL, "synth_up2: null input");
    ATMVFI_REQUIRE(p->B <= 16, ATMVFI_EINVAL, "synth_up2: at most 16 pairs per call (got %d)", p->B);
    ATMVFI_REQUIRE(synth_up2_shape_ok(p->B, p->h, p->w), ATMVFI_EINVAL, "synth_up2: bad shape (B %d, h %d, w %d)", p->B, p->h, p->w);
    ATMVFI_REQUIRE(p->S0 >= 1 && p->S1 >= 1, ATMVFI_EINVAL, "synth_up2: empty frame store");
    ATMVFI_REQUIRE(p->dst_f32 || p->dst_u8, ATMVFI_EINVAL, "synth_up2: no output requested (dst_f32, dst_u8 or both)");
    ATMVFI_REQUIRE((p->f0_out == nullptr) == (p->f1_out == nullptr), ATMVFI_EINVAL, "synth_up2: the flow outputs come in pairs");
    const int B = p->B, H = 2 * p->h, W = 2 * p->w;
    const long long hw = (long long)H * W, qhw = (long long)p->h * p->w;
    SynthUp2Args a{};
    for (int b = 0; b < B; ++b) {
        a.s0[b] = p->slots0 ? p->slots0[b] : b;
        a.s1[b] = p->slots1 ? p->slots1[b] : b;
        ATMVFI_REQUIRE(a.s0[b] >= 0 && a.s0[b] < p->S0 && a.s1[b] >= 0 && a.s1[b] < p->S1, ATMVFI_EINVAL,
                       "synth_up2: pair %d names frames (%d, %d) outside the stores of %d and %d", b, a.s0[b], a.s1[b], p->S0, p->S1);
    }
    if (p->dst_u8)
        ATMVFI_REQUIRE(p->pad_top >= 0 && p->pad_left >= 0 && p->hh >= 1 && p->ww >= 1 && (long long)p->pad_top + p->hh <= H &&
                           (long long)p->pad_left + p->ww <= W, ATMVFI_EINVAL,
                       "synth_up2: the window %d x %d at (%d, %d) is outside the %d x %d canvas", p->hh, p->ww, p->pad_top, p->pad_left, H, W);
    const bool can_stage = W % 4 == 0 && atmvfi::aligned16(p->store0) && atmvfi::aligned16(p->store1);
    ATMVFI_REQUIRE(p->path >= 0 && p->path <= 2, ATMVFI_EINVAL, "synth_up2: path must be 0 (auto), 1 (gathers) or 2 (staged), got %d", p->path);
    ATMVFI_REQUIRE(p->path != 2 || can_stage, ATMVFI_EINVAL, "synth_up2: the staged path needs 2w %% 4 == 0 and 16-byte aligned stores (got 2w = %d)", W);
    const ByteRange in[8] = {{p->it_sum, B * 3 * qhw * 4, "it_sum"}, {p->it0, B * 3 * qhw * 4, "it0"}, {p->it1, B * 3 * qhw * 4, "it1"},
                             {p->flow0, B * 2 * qhw * 4, "flow0"}, {p->flow1, B * 2 * qhw * 4, "flow1"}, {p->m1, B * qhw * 4, "m1"},
                             {p->store0, p->S0 * 3 * hw * 4, "store0"}, {p->store1, p->S1 * 3 * hw * 4, "store1"}};
    const ByteRange out[5] = {{p->dst_f32, B * 3 * hw * 4, "dst_f32"}, {p->dst_u8, p->dst_u8 ? (long long)B * p->hh * p->ww * 3 : 0, "dst_u8"},
                              {p->f0_out, B * 2 * hw * 4, "f0_out"}, {p->f1_out, B * 2 * hw * 4, "f1_out"}, {p->m_out, B * hw * 4, "m_out"}};
    for (int o = 0; o < 5; ++o) {
        for (int i = 0; i < 8; ++i)
            ATMVFI_REQUIRE(!ranges_overlap(out[o], in[i]), ATMVFI_EINVAL, "synth_up2: %s overlaps %s", out[o].name, in[i].name);
        for (int j = 0; j < o; ++j)
            ATMVFI_REQUIRE(!ranges_overlap(out[o], out[j]), ATMVFI_EINVAL, "synth_up2: %s overlaps %s", out[o].name, out[j].name);
    }
    const long long tiles = warp_tiles(B, H, W);
    ATMVFI_REQUIRE(tiles < (1ll << 31), ATMVFI_EINVAL, "synth_up2: grid too large");
    a.it_sum = p->it_sum; a.it0 = p->it0; a.it1 = p->it1; a.flow0 = p->flow0; a.flow1 = p->flow1; a.m1 = p->m1;
    a.store0 = p->store0; a.store1 = p->store1;
    a.dst = p->dst_f32; a.f0o = p->f0_out; a.f1o = p->f1_out; a.mo = p->m_out;
    a.dst_u8 = (unsigned char*)p->dst_u8;
    a.h = p->h; a.w = p->w;
    a.pad_top = p->pad_top; a.pad_left = p->pad_left; a.hh = p->hh; a.ww = p->ww; a.bgr = p->bgr;
    // path 0 is the gathering instance: measured faster than the staged one at small flows and level with it at large ones
    // (profiles/scaled_bench.txt); the staged instance runs on request
    if (p->path == 2)
        hipLaunchKernelGGL(synth_up2_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(synth_up2_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
    return atmvfi::check_launch("synth_up2");
}
