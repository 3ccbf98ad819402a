// What the plane-input GEMM engines share (gemm_pp.hip: 256 x 128 tiles, ping-pong wave groups, persistent grid; gemm_duo.hip: 128 x 128
// / 128 x 64 tiles, two or three workgroups per CU): the small LDS / DMA helpers (also used by gemm_split.hip and gemm_f16x3.hip), the
// CONV-mode operand addressing, the epilogue behind the LDS transposition, and the launchers' prologue -- one copy each.
// The yardsticks stay independent ON PURPOSE: the epilogue of gemm_split_kernel (the reference schedule the bit-identity test compares
// against), gemm_splitk_reduce_kernel and gemm_f16x3.hip's epilogue are separate implementations on gemm_finish_store4 (gemm_common.h).
#pragma once
#include "common.h"
#include "gemm_common.h"
#include "plane_common.h"      // f16x8, LO_UNSCALE, swz64, dma16, wait_vm

__device__ __forceinline__ void lds_write16f(unsigned addr, const f32x4& v) {
    asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read16f(f32x4& d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}

namespace atmvfi {

// ---- CONV mode (strided / dilated / 1x1 convolutions, network_base.py:20-25, 73-85): k-step = (tap, 32-channel chunk); GEMM row m is
// output pixel (n, oy, ox) and its operand row at tap (ky, kx) is input pixel (n, oy*stride - pad + ky*dil, ox*stride - pad + kx*dil),
// or the planes' zero row N*H*W when that falls outside the image -- the same DMA with a per-lane source row.
struct PlaneConvWalk {
    int crow[2], cyx[2];      // per lane and A row: the input row of tap (0, 0), and its (y, x) packed into one register
    int ky, kx, chunk;        // wave-uniform: tap and chunk of the stage that goes out next
};
// (both helpers take the descriptor by reference: by value gemm_duo's 64-column CONV kernel needs a 129th register and loses a workgroup
// per CU)
// Row setup: GEMM row m -> (cyx, crow) of the lane's A row i.  LAUNDER: the divisors go through an empty asm: otherwise hipcc hoists
// their reciprocals out of gemm_pp's tile loop and keeps them in vector registers across the k-loop, which is at the 256-register limit.
template <bool LAUNDER>
__device__ __forceinline__ void plane_conv_row(const GemmDev& a, int m, int i, PlaneConvWalk& cv) {
    int hw = a.Ho * a.Wo, wo = a.Wo;
    if constexpr (LAUNDER) asm volatile("" : "+s"(hw), "+s"(wo));
    const int n = (int)((unsigned)m / (unsigned)hw);
    const int rem = m - n * hw;
    const int oy = rem / wo, ox = rem - oy * wo;
    const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
    cv.cyx[i] = (iy0 << 16) | (ix0 & 0xffff);
    cv.crow[i] = (n * a.H + iy0) * a.W + ix0;
}
// The four A pieces of one stage (hi and lo plane of the lane's two rows; the second row's piece ROW2 bytes behind the first), then
// the step to the next (tap, chunk).  pa_hi / pa_lo: the first source's planes; a_step: bytes per chunk in them.
template <int A_LO, int ROW2>
__device__ __forceinline__ void plane_conv_issue(const GemmDev& a, PlaneConvWalk& cv, const unsigned char* pa_hi, const unsigned char* pa_lo,
                                                 long long a_step, int zero_row, unsigned ls16, unsigned char* dst) {
    // plane pointers of this stage's chunk: the first source, or (channels >= 32 * split_chunks) the second one
    const bool second = cv.chunk >= a.split_chunks;
    const unsigned char* bh = second ? reinterpret_cast<const unsigned char*>(a.a_hi2) + (long long)(cv.chunk - a.split_chunks) * a.in_ld2 * 64
                                     : pa_hi + (long long)cv.chunk * a_step;
    const unsigned char* bl = second ? reinterpret_cast<const unsigned char*>(a.a_lo2) + (long long)(cv.chunk - a.split_chunks) * a.in_ld2 * 64
                                     : pa_lo + (long long)cv.chunk * a_step;
    const int dyo = cv.ky * a.dil, dxo = cv.kx * a.dil;
    unsigned off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int iy = (cv.cyx[i] >> 16) + dyo, ix = (int)(short)cv.cyx[i] + dxo;
        const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        const int row = ok ? cv.crow[i] + dyo * a.W + dxo : zero_row;
        off[i] = (unsigned)row * 64u + ls16;
    }
    dma16(bh + off[0], dst);
    dma16(bh + off[1], dst + ROW2);
    dma16(bl + off[0], dst + A_LO);
    dma16(bl + off[1], dst + A_LO + ROW2);
    if (++cv.chunk == a.cpt32) {
        cv.chunk = 0;
        if (++cv.kx == a.kw) { cv.kx = 0; ++cv.ky; }
    }
}

// ---- epilogue of a BM x BN tile whose waves own 16 MI x 64 outputs each (wave (wm, wn) of the tile at (m0, n0)).
// After the k-loop lane (r, g) holds, of its MFMA tiles (i, j), GEMM row 16 MI wm + 16 i + r and columns 64 wn + 16 j + 4 g .. + 3: a
// 16-byte store per lane in that layout touches 16 rows x 64 B per instruction, and the store path then takes 52 cycles per
// instruction where 256 contiguous bytes per 16 lanes take 15 (tools/probes/store_probe.hip: 19.6 against 67.5 B/clk/CU; 8 rows x
// 128 B is no better than 16 x 64 B) -- 8 k of a 42 k-cycle K = 384 tile.  So the kernels fold (acc + cor / 1024) and TRANSPOSE every
// 16-row slab i THROUGH LDS, each in its own layout, before they call this: four ds_write_b128 (lane (r, g): row r, 16-byte slot
// 4 j + g) and four ds_read_b128 (lane (r, g): row 4 q + g, slot r) leave lane (r, g) with acc[i][q] = GEMM rows 16 MI wm + 16 i +
// 4 q + g, q = 0..3, columns 64 wn + 4 r .. + 3 -- the 16 lanes of a row cover 256 contiguous bytes, residual loads included.
// Per-tile constants (cst: gemm_dma_consts<BN> + the tile's BM row-map entries): bias / slope of the lane's four columns (two LDS
// reads per tile instead of two per vector); row-map entries from LDS; (LINEAR with a residual whose width is a multiple of 4: every
// case of the network) all residual vectors in one batch of unconditional loads before the first store (one wait per tile; vmcnt
// counts stores on gfx9, so a wait per row would drain the previous row's stores).
// `a` by value: by reference hipcc re-selects the descriptor's pointers per use (17-33 more s_cmp / s_cselect pairs per kernel).
// after_residuals: called once between the residual batch and the stores (the stamp build's phase boundary).
struct NoHook {
    __device__ __forceinline__ void operator()() const {}
};
template <bool CONVM, int MI, int BM, int BN, typename Hook = NoHook>
__device__ __forceinline__ void plane_gemm_epilogue(const GemmDev a, f32x4 (&acc)[MI][4], const float* cst, int m0, int n0, int M, int wm, int wn,
                                                    int r, int g, Hook after_residuals = Hook{}) {
    constexpr int WROWS = 16 * MI;
    const bool mapped = a.out_row_map && a.mode == ATMVFI_GEMM_LINEAR;
    const int cl = 64 * wn + 4 * r;                          // the lane's four columns inside the column block
    const int nb = n0 + cl;
    const ChanPos cp = gemm_chan_pos(a, nb);
    const f32x4 bvec = *reinterpret_cast<const f32x4*>(cst + cl);
    const f32x4 pvec = *reinterpret_cast<const f32x4*>(cst + BN + cl);
    const int mrow = m0 + WROWS * wm + g;                    // row of (i, q) = (0, 0); (i, q) adds 16 i + 4 q
    int ro[MI][4];              // output row: the row map's entry, or (unmapped) the row itself; < 0: nothing to store
    if (mapped) {                 // (the test outside the loops: inside, hipcc makes it a scalar branch per row)
        const int* mp = reinterpret_cast<const int*>(cst + gemm_const_floats(BN)) + WROWS * wm + g;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) ro[i][q] = (mrow + 16 * i + 4 * q) < M ? mp[16 * i + 4 * q] : -1;
    } else {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = mrow + 16 * i + 4 * q;
                ro[i][q] = m < M ? m : -1;
            }
    }
    const bool vec_res = !CONVM && a.residual && (a.Cout & 3) == 0 && a.mode != ATMVFI_GEMM_DECONV;
    f32x4 res[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) res[i][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (vec_res && a.fit32 && m0 + BM <= M) {
        // (all rows live: 32-bit offsets from a scalar base, stepped by 4 rows)
        const unsigned char* rb = reinterpret_cast<const unsigned char*>(a.residual);
        unsigned voff = nb < a.Cout ? ((unsigned)mrow * (unsigned)a.res_ld + (unsigned)nb) * 4u : 0u;
        const unsigned step = nb < a.Cout ? (unsigned)a.res_ld * 16u : 0u;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                res[i][q] = *reinterpret_cast<const f32x4*>(rb + voff);
                voff += step;
            }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(res[i][q]));
    } else if (vec_res) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = mrow + 16 * i + 4 * q;
                const float* p = (ro[i][q] >= 0 && nb < a.Cout) ? a.residual + m * (long long)a.res_ld + nb : a.residual;
                res[i][q] = *reinterpret_cast<const f32x4*>(p);
            }
        // every vector is "used" here, dead rows' too: a load left pending on some path makes hipcc guard the next tile's first
        // write to its register with s_waitcnt vmcnt(0), which would also wait for this tile's stores
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(res[i][q]));
    }
    // DECONV: the lane's rows are 4 apart: (image, y, x) of the first one by division, the others by stepping
    int dn = 0, dy = 0, dx = 0;
    if (a.mode == ATMVFI_GEMM_DECONV) {
        const int hw = a.H * a.W;
        dn = (int)((unsigned)mrow / (unsigned)hw);
        const int rem = mrow - dn * hw;
        dy = rem / a.W;
        dx = rem - dy * a.W;
    }
    // (two copies of the store loop under a uniform branch: with the ragged-width residual loads as a conditional inside one
    // loop, hipcc puts their s_waitcnt vmcnt(0) into the shared block, i.e. in front of every store of the common case too)
    auto store_rows = [&](auto ragged_tag) {
        constexpr bool RAGGED = decltype(ragged_tag)::value;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = mrow + 16 * i + 4 * q;
                float* orow = nullptr;
                long long prow = 0;
                int pc0 = a.out_c0;
                if (a.mode == ATMVFI_GEMM_DECONV) {
                    prow = ((long long)dn * a.Ho + 2 * dy) * a.Wo + 2 * dx;
                    orow = a.out + prow * a.out_ld;
                    dx += 4;                                  // next row of this lane
                    while (dx >= a.W) { dx -= a.W; if (++dy == a.H) { dy = 0; ++dn; } }
                } else {
                    const int rr = ro[i][q] < 0 ? 0 : ro[i][q];
                    prow = rr;
                    long long off = (long long)rr * a.out_ld;
                    if (a.out_rpg > 0) {
                        const int gi = (int)((unsigned)rr / (unsigned)a.out_rpg);
                        prow = rr - gi * a.out_rpg;
                        off = gi * a.out_gstride + prow * (long long)a.out_ld;
                        pc0 += gi * a.out_gc;
                    }
                    orow = a.out + off;
                }
                if (ro[i][q] >= 0) {
                    f32x4 rv = res[i][q];
                    if constexpr (RAGGED) rv = gemm_load_residual4(a.residual + m * (long long)a.res_ld, cp);
                    gemm_finish_store4(a, orow, prow, pc0, cp, acc[i][q], bvec, pvec, rv);
                }
            }
    };
    after_residuals();
    // Fast variants for the network's three output shapes, chosen once per tile: inside them nothing is decided per row (the
    // generic loop above spends ~10 scalar / exec branches per row on mode, groups, sinks and ragged widths: 11 k cycles per
    // tile for 16 rows per lane).  All have full 4-channel vectors (Cout % 4 == 0, or DECONV whose position blocks are padded
    // to 4) and do the arithmetic of gemm_finish_store4 in its order: + bias, PReLU (slope 1 when absent), + residual.
    // (the fast loops exist twice, with and without a PReLU: the select costs 14 of a row's ~30 VALU instructions, and the
    // epilogue of a group is VALU-bound -- one wave per SIMD beside the other group's MFMAs)
    auto fast_rows = [&](auto prelu_tag) {
        constexpr bool PRELU = decltype(prelu_tag)::value;
        auto finish = [&](int i, int q, bool with_res = true) -> f32x4 {
            f32x4 v = acc[i][q] + bvec;
            if constexpr (PRELU) {
                v.x = v.x > 0.f ? v.x : pvec.x * v.x;
                v.y = v.y > 0.f ? v.y : pvec.y * v.y;
                v.z = v.z > 0.f ? v.z : pvec.z * v.z;
                v.w = v.w > 0.f ? v.w : pvec.w * v.w;
            }
            if constexpr (CONVM) return v;           // convolutions have no residual operand
            else return with_res ? v + res[i][q] : v;
        };
        if (a.mode != ATMVFI_GEMM_DECONV && !a.out_hi && a.fit32 && m0 + BM <= M) {
            // fp32 rows, every row of the tile live, no map: one 32-bit byte offset per lane, stepped by 4 rows -- a row costs
            // its arithmetic (bias, residual) and one add; stores with a scalar base
            if (nb < a.Cout) {
                unsigned char* ob = reinterpret_cast<unsigned char*>(a.out);
                unsigned voff = ((unsigned)mrow * (unsigned)a.out_ld + (unsigned)nb) * 4u;
                const unsigned step = (unsigned)a.out_ld * 16u;
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        *reinterpret_cast<f32x4*>(ob + voff) = finish(i, q);
                        voff += step;
                    }
            }
        } else if (a.mode != ATMVFI_GEMM_DECONV && !a.out_hi) {
            // fp32 rows (qkv, fc1, proj with its row map and residual, fc2, fusion projections; convolutions)
            float* obase = a.out + nb;
            const bool col_ok = nb < a.Cout;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = finish(i, q);
                    const unsigned long long off = (unsigned long long)(unsigned)ro[i][q] * (unsigned)a.out_ld;
                    if (ro[i][q] >= 0 && col_ok) *reinterpret_cast<f32x4*>(obase + off) = v;
                }
        } else if (a.mode != ATMVFI_GEMM_DECONV) {
            // plane sink, with or without fp32 rows (optionally a grouped [G, R, C] view): the last fc2 of a motion branch,
            // strided / 1x1 convolutions between plane maps
            const unsigned rpg = a.out_rpg > 0 ? (unsigned)a.out_rpg : 0x7fffffffu;
            const RowSink sink{nullptr, 0, a.out_hi, a.out_lo, a.out_plane_rows};
            const bool col_ok = nb < a.Cout;
            // ungrouped sink whose planes fit 32-bit byte offsets (every strided / 1x1 conv between plane maps): the lane's
            // channel group fixes a pointer into each plane once per tile, a row costs a shift (the grouped form divides
            // every row by the group size: ~25 VALU instructions of a VALU-bound epilogue)
            auto rows32 = [&](auto f32_tag) {
                constexpr bool F32 = decltype(f32_tag)::value;
                const int c = a.out_c0 + nb;
                const long long cpart = ((long long)(c >> 5) * a.out_plane_rows) * 32 + (c & 31);
                unsigned char* ph = reinterpret_cast<unsigned char*>(a.out_hi + cpart);
                unsigned char* pl = reinterpret_cast<unsigned char*>(a.out_lo + cpart);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 v = finish(i, q);
                        const unsigned rr = ro[i][q] < 0 ? 0u : (unsigned)ro[i][q];
                        if (ro[i][q] >= 0 && col_ok) {
                            if constexpr (F32) *reinterpret_cast<f32x4*>(a.out + (unsigned long long)rr * (unsigned)a.out_ld + nb) = v;
                            f16x2 h0, l0, h1, l1;
                            split_pair((f32x2){v.x, v.y}, h0, l0);
                            split_pair((f32x2){v.z, v.w}, h1, l1);
                            *reinterpret_cast<f16x4*>(ph + (rr << 6)) = (f16x4){h0.x, h0.y, h1.x, h1.y};
                            *reinterpret_cast<f16x4*>(pl + (rr << 6)) = (f16x4){l0.x, l0.y, l1.x, l1.y};
                        }
                    }
            };
            auto rows = [&](auto f32_tag) {
                constexpr bool F32 = decltype(f32_tag)::value;
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 v = finish(i, q);
                        const unsigned rr = ro[i][q] < 0 ? 0u : (unsigned)ro[i][q];
                        const unsigned gi = rr / rpg;
                        const long long prow = rr - gi * rpg;
                        if (ro[i][q] >= 0 && col_ok) {
                            if constexpr (F32) *reinterpret_cast<f32x4*>(a.out + gi * a.out_gstride + prow * (long long)a.out_ld + nb) = v;
                            sink_store4(sink, prow, a.out_c0 + (int)gi * a.out_gc + nb, v);
                        }
                    }
            };
            if (a.out_rpg == 0 && a.pfit32) {
                if (a.out) rows32(std::true_type{});
                else rows32(std::false_type{});
            } else if (a.out) rows(std::true_type{});
            else rows(std::false_type{});
        } else {
            // ConvTranspose2d 2x2 / stride 2 into a plane sink (decoder and U-Net stages): column -> (position, channel) is a
            // lane constant; the lane's rows are 4 input pixels apart: (image, y, x) of the first by division, the others by
            // stepping
            const RowSink sink{nullptr, 0, a.out_hi, a.out_lo, a.out_plane_rows};
            const int hw = a.H * a.W;
            int dn = (int)((unsigned)mrow / (unsigned)hw);
            const int rem = mrow - dn * hw;
            int dy = rem / a.W;
            int dx = rem - dy * a.W;
            const int qoff = (cp.q >> 1) * a.Wo + (cp.q & 1);
            const int pc = a.out_c0 + cp.co;
            if (a.pfit32) {
                // 32-bit row offsets from the lane's chunk pointers.  Output row index of (image dn, input row dy, input
                // column 0) is (dn Ho + 2 dy) Wo, and because Ho = 2 H it simply grows by 2 Wo whenever the stepped input
                // column wraps -- across images too: no (dn, dy) bookkeeping, no 64-bit products per row.
                const long long cpart = ((long long)(pc >> 5) * a.out_plane_rows) * 32 + (pc & 31);
                unsigned char* ph = reinterpret_cast<unsigned char*>(a.out_hi + cpart);
                unsigned char* pl = reinterpret_cast<unsigned char*>(a.out_lo + cpart);
                unsigned rowbase = ((unsigned)dn * (unsigned)a.Ho + 2u * (unsigned)dy) * (unsigned)a.Wo + (unsigned)qoff;
                const unsigned rstep = 2u * (unsigned)a.Wo;
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        // (no residual on this path; channels past Cout inside the group of 4 are already zero: their weight
                        // rows and their bias are, and PReLU keeps a zero)
                        const f32x4 v = finish(i, q, false);
                        const unsigned boff = (rowbase + 2u * (unsigned)dx) << 6;
                        if (ro[i][q] >= 0 && cp.nvalid > 0) {
                            f16x2 h0, l0, h1, l1;
                            split_pair((f32x2){v.x, v.y}, h0, l0);
                            split_pair((f32x2){v.z, v.w}, h1, l1);
                            *reinterpret_cast<f16x4*>(ph + boff) = (f16x4){h0.x, h0.y, h1.x, h1.y};
                            *reinterpret_cast<f16x4*>(pl + boff) = (f16x4){l0.x, l0.y, l1.x, l1.y};
                        }
                        dx += 4;                                  // next row of this lane (W >= 4: one wrap at most)
                        const bool wrap = dx >= a.W;
                        dx = wrap ? dx - a.W : dx;
                        rowbase += wrap ? rstep : 0u;
                    }
            } else
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v = finish(i, q);
                    v.y = cp.nvalid > 1 ? v.y : 0.f;            // channels past Cout inside the group of 4: the planes' pad channels
                    v.z = cp.nvalid > 2 ? v.z : 0.f;
                    v.w = cp.nvalid > 3 ? v.w : 0.f;
                    const long long prow = ((long long)dn * a.Ho + 2 * dy) * a.Wo + 2 * dx + qoff;
                    if (ro[i][q] >= 0 && cp.nvalid > 0) sink_store4(sink, prow, pc, v);
                    dx += 4;                                      // next row of this lane (W >= 4: one wrap at most)
                    const bool wrap = dx >= a.W;
                    dx = wrap ? dx - a.W : dx;
                    dy = wrap ? dy + 1 : dy;
                    const bool wrap2 = dy >= a.H;
                    dy = wrap2 ? 0 : dy;
                    dn = wrap2 ? dn + 1 : dn;
                }
        }
    };
    const bool c4 = (a.Cout & 3) == 0;
    const bool fast = (a.mode != ATMVFI_GEMM_DECONV && c4 && (a.out_hi || (a.out && a.out_rpg == 0))) ||
                      (a.mode == ATMVFI_GEMM_DECONV && !a.out && a.out_hi && a.W >= 4 && !a.residual);
    if (fast) {
        if (a.prelu) fast_rows(std::true_type{});
        else fast_rows(std::false_type{});
    } else if (a.residual && !vec_res) {
        store_rows(std::true_type{});
    } else {
        store_rows(std::false_type{});
    }
}

// ---- launcher prologue of both engines (`engine`: its name in the messages): the 32-bit limits the kernels' address arithmetic rests
// on, the 32-bit fast-path predicates, and the XCD-aware grid of BM x BN tiles (virtual blocks incl. XCD padding).
inline int plane_gemm_prepare(const char* engine, GemmDev& d, int ngemm, int BM, int BN) {
    ATMVFI_REQUIRE((long long)d.in_ld * 64 < (1ll << 32) && (long long)d.wrows * 64 < (1ll << 32) &&
                       (!d.a_hi2 || (long long)d.in_ld2 * 64 < (1ll << 32)) && d.M < (1ll << 26), ATMVFI_EINVAL,
                   "%s: plane rows x 64 bytes must fit 32 bits (got %d rows)", engine, d.in_ld);
    if (d.mode == ATMVFI_GEMM_CONV)
        ATMVFI_REQUIRE(d.H < 32768 && d.W < 32768, ATMVFI_EINVAL, "%s: CONV mode packs (y, x) into 16 bits each", engine);
    d.dbg = 0;
    d.pfit32 = d.out_hi && (long long)d.out_plane_rows * 64 < (1ll << 32);
    d.fit32 = d.out && !d.out_row_map && d.out_rpg == 0 && d.mode != ATMVFI_GEMM_DECONV && (d.M + 1) * (long long)d.out_ld * 4 < (1ll << 32) &&
               (!d.residual || (d.M + 1) * (long long)d.res_ld * 4 < (1ll << 32));
    d.nblocks = (ngemm + BN - 1) / BN;
    const long long mgroups = (ceil_div64(d.M, BM) + 7) / 8;
    ATMVFI_REQUIRE(mgroups * 8 * d.nblocks < (1LL << 31), ATMVFI_EINVAL, "%s: grid too large", engine);
    d.vblocks = (int)(mgroups * 8 * d.nblocks);
    return ATMVFI_OK;
}

}  // namespace atmvfi
