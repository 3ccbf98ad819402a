// LDS-DMA GEMM on split-plane activations, TWO WORKGROUPS PER CU (gfx950): the same contract and the same arithmetic as gemm_pp.hip
// (x = hi + lo'/1024 in fp16, three v_mfma_f32_16x16x32_f16 per product into two fp32 accumulators, k ascending, per accumulator the same
// order of products: bit-identical results), the same 64 x 64 wave tile, and gemm_plane.h's epilogue, CONV-mode operand addressing and
// launcher prologue, which the two engines share -- but 128 x 128 tiles on 256 threads, two 32-KiB LDS stages, one tile per workgroup and no phase control: two workgroups share a CU, so one's prologue, fragment reads and
// epilogue (a third of a K = 384 tile in gemm_pp.hip, where all eight waves of the CU are in the epilogue together) run under the other's
// MFMAs.  Chosen per launch by launch_gemm_split (gemm_split.hip); atmvfi_gemm_params.tile_wn = -2 / -4 force its 128- / 64-column form
// (A/B against gemm_pp.hip: tools/bench_split_ab.py, tools/duo_rule.py, tools/narrow_ab.py).
#include "gemm_plane.h"

namespace {

using atmvfi::GemmDev;

constexpr int BM = 128;
// BN = 128: 4 waves as 2 x 2 of 64 x 64; BN = 64 (layers of at most 64 columns: half of a 128-column tile would be padding): 4 waves as
// 4 x 1 of 32 x 64, 24-KiB stages, three workgroups per CU
constexpr int stage_bytes(int BN) { return (2 * BM + 2 * BN) * 64; }   // [A hi 128 rows][A lo][W hi BN rows][W lo], 64 B per row
constexpr int A_LO = BM * 64, W_HI = 2 * BM * 64;
constexpr int cst_floats(int BN) { return atmvfi::gemm_const_floats(BN) + BM; }      // bias / slope of the column block + the tile's row-map entries

#ifdef ATMVFI_STAMP
// Diagnostic build only (`make stamp`, tools/stamp_duo.py): shader-clock sums per phase of the k-loop, per wave
static unsigned long long* g_duo_stamp = nullptr;
extern "C" void atmvfi_debug_set_duo_stamp_buffer(void* p) { g_duo_stamp = (unsigned long long*)p; }
#define DUO_SUB(k) do { if (a.stamp) { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); sub[k] += t_ - sub_t; sub_t = t_; __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define DUO_SUB(k) do { } while (0)
#endif

// X3: the three-term product (the default).  X3 == false (ATMVFI_PREC_F16): hi(x) * hi(w) alone -- no lo' fragment reads, a third of the
// MFMAs, no `cor`; DMA of both planes, stages, counted waits and barriers are the same source.  A split-K range's raw sum is `acc`.
template <bool CONVM, int BN, bool X3>
__global__ __launch_bounds__(256, 2) void gemm_duo_kernel(const GemmDev a) {
    constexpr int STAGE = stage_bytes(BN), W_LO = W_HI + BN * 64;
    constexpr int MI = BN == 128 ? 4 : 2;           // 16-row MFMA tiles per wave along M
    constexpr int NWN = BN / 64;                    // waves along N (64 columns each)
    constexpr int WROWS = 16 * MI;
    constexpr int PIW = BN / 64;                    // 16-row DMA pieces of a W plane per wave (A: always 2)
    fp16_saturate_on();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15;
    const int g = lane >> 4;
    const int wm = wave / NWN, wn = wave % NWN;

    // XCD-aware tile order of gemm_pp.hip (virtual block v: xcd = v & 7, slot = v >> 3, row tile = (slot / nblocks) * 8 + xcd, column
    // block = slot % nblocks: the column blocks of one row tile meet in one L2), one tile per workgroup
    const int M = (int)a.M;
    int m0, n0;
    {
        const int v = blockIdx.x;
        const int xcd = v & 7, slot = v >> 3;
        const int mgrp = slot / a.nblocks;
        m0 = (mgrp * 8 + xcd) * BM;
        n0 = (slot - mgrp * a.nblocks) * BN;
    }
    if (m0 >= M) return;
    float* cst_w = reinterpret_cast<float*>(smem + 2 * STAGE);
    const float* cst = cst_w;

    // ---- DMA pieces of this wave: A rows (i * 4 + wave) * 16 + lane / 4 (i = 0, 1) of both planes, W rows the same.  LDS image of a
    // piece: wave-uniform base + lane * 16 B; the slot swizzle goes on the SOURCE address.
    const unsigned ls16 = (unsigned)(((lane & 3) ^ swz64(lane >> 2)) << 4);
    unsigned aoff[2], wsoff[2];
    atmvfi::PlaneConvWalk cv;             // CONV mode (gemm_plane.h)
    cv.ky = cv.kx = cv.chunk = 0;
    const int zero_row = a.in_N * a.H * a.W;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = m0 + (i * 4 + wave) * 16 + (lane >> 2);
        if (m >= M) m = M - 1;
        if constexpr (CONVM) atmvfi::plane_conv_row<false>(a, m, i, cv);
        else aoff[i] = (unsigned)m * 64u + ls16;
        if (i < PIW) {
            int n = n0 + (i * 4 + wave) * 16 + (lane >> 2);
            if (n >= a.wrows) n = a.wrows - 1;
            wsoff[i] = (unsigned)n * 64u + ls16;
        }
    }
    const unsigned char* pa_hi = reinterpret_cast<const unsigned char*>(a.a_hi);
    const unsigned char* pa_lo = reinterpret_cast<const unsigned char*>(a.a_lo);
    const unsigned char* pw_hi = reinterpret_cast<const unsigned char*>(a.w_hi);
    const unsigned char* pw_lo = reinterpret_cast<const unsigned char*>(a.w_lo);
    const long long a_step = (long long)a.in_ld * 64, w_step = (long long)a.wrows * 64;
    int nk = a.nchunks32;
    if (a.ksplit > 1) {
        // this workgroup's range of k-steps: the first (nk mod ksplit) ranges take one more
        const int sp = blockIdx.y;
        const int per = nk / a.ksplit, rem = nk - per * a.ksplit;
        const int u0 = sp * per + (sp < rem ? sp : rem);
        nk = per + (sp < rem ? 1 : 0);
        pw_hi += (long long)u0 * w_step;
        pw_lo += (long long)u0 * w_step;
        if constexpr (CONVM) {
            const int tap = u0 / a.cpt32;
            cv.chunk = u0 - tap * a.cpt32;
            cv.ky = tap / a.kw;
            cv.kx = tap - cv.ky * a.kw;
        } else {
            pa_hi += (long long)u0 * a_step;
            pa_lo += (long long)u0 * a_step;
        }
    }
    auto issue_stage = [&](int buf) {                               // 4 + 2 PIW pieces per wave
        unsigned char* dst = smem + buf * STAGE + wave * 1024;
        if constexpr (CONVM) {
            atmvfi::plane_conv_issue<A_LO, 4 * 1024>(a, cv, pa_hi, pa_lo, a_step, zero_row, ls16, dst);
        } else {
            dma16(pa_hi + aoff[0], dst);
            dma16(pa_hi + aoff[1], dst + 4 * 1024);
            dma16(pa_lo + aoff[0], dst + A_LO);
            dma16(pa_lo + aoff[1], dst + A_LO + 4 * 1024);
            pa_hi += a_step;
            pa_lo += a_step;
        }
        dma16(pw_hi + wsoff[0], dst + W_HI);
        if constexpr (PIW == 2) dma16(pw_hi + wsoff[1], dst + W_HI + 4 * 1024);
        dma16(pw_lo + wsoff[0], dst + W_LO);
        if constexpr (PIW == 2) dma16(pw_lo + wsoff[1], dst + W_LO + 4 * 1024);
        pw_hi += w_step;
        pw_lo += w_step;
    };
    // per-tile constants by LDS-DMA, one piece per wave (4 waves: bias and slope halves; the row map's 128 entries by waves 0-1 again)
    {
        atmvfi::gemm_dma_consts<BN>(a, n0, cst_w, wave, lane);
        if (a.out_row_map && a.mode == ATMVFI_GEMM_LINEAR) {
            int m = m0 + (wave & 1) * 64 + lane;
            if (m >= M) m = M - 1;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.out_row_map + m),
                                             (__attribute__((address_space(3))) void*)(cst_w + atmvfi::gemm_const_floats(BN) + (wave & 1) * 64), 4, 0, 0);
        } else {
            atmvfi::gemm_dma_consts<BN>(a, n0, cst_w, wave, lane);
        }
    }

    f32x4 acc[MI][4];
    RegsIf<X3, f32x4[MI][4]> cor;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if constexpr (X3) cor[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#ifdef ATMVFI_STAMP
    unsigned long long sub[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sub_t = 0, t_begin = 0;
    if (a.stamp) { t_begin = sub_t = __builtin_amdgcn_s_memtime(); }
#endif
    issue_stage(0);
    if (nk > 1) issue_stage(1);
    DUO_SUB(0);
    f16x8 xh[MI], wh[4];
    RegsIf<X3, f16x8[MI]> xl;
    RegsIf<X3, f16x8[4]> wl;
    const unsigned xfrag = lds_offset(smem) + (unsigned)((WROWS * wm + r) * 64 + ((g ^ swz64(r)) << 4));
    const unsigned wfrag = lds_offset(smem) + (unsigned)(W_HI + (64 * wn + r) * 64 + ((g ^ swz64(r)) << 4));
    for (int u = 0; u < nk; ++u) {
        // this wave's pieces of stage u have landed (8 newer ones, stage u + 1, may stay in flight), then everybody's
        if (u + 1 < nk) wait_vm<4 + 2 * PIW>();
        else wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        DUO_SUB(1);
        const unsigned off = (unsigned)((u & 1) * STAGE);
        static_for<0, MI>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            lds_read16<i * 1024>(xh[i], xfrag + off);
            if constexpr (X3) lds_read16<i * 1024 + A_LO>(xl[i], xfrag + off);
        });
        static_for<0, 4>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            lds_read16<j * 1024>(wh[j], wfrag + off);
            if constexpr (X3) lds_read16<j * 1024 + BN * 64>(wl[j], wfrag + off);
        });
        if constexpr (X3) {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh[0]), "+v"(xh[1]), "+v"(xl[0]), "+v"(xl[1]));
            if constexpr (MI == 4) asm volatile("" : "+v"(xh[2]), "+v"(xh[3]), "+v"(xl[2]), "+v"(xl[3]));
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(wh[j]), "+v"(wl[j]));
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh[0]), "+v"(xh[1]));
            if constexpr (MI == 4) asm volatile("" : "+v"(xh[2]), "+v"(xh[3]));
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(wh[j]));
        }
        DUO_SUB(2);
        __builtin_amdgcn_s_barrier();                   // every wave has its fragments: the buffer may be refilled
        DUO_SUB(3);
        if (u + 2 < nk) issue_stage(u & 1);
        DUO_SUB(4);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (X3) cor[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j], xh[i], cor[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xh[i], acc[i][j], 0, 0, 0);
            }
        if constexpr (X3) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) cor[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xl[i], cor[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        DUO_SUB(5);
    }
    {
        __builtin_amdgcn_s_barrier();                       // every wave is past its last fragment read (the transposition reuses stage 0)
        // ---- epilogue (gemm_plane.h: why and how the slabs are transposed, and everything behind the transposition)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (X3) acc[i][j] = acc[i][j] + cor[i][j] * LO_UNSCALE;
                asm volatile("" : "+v"(acc[i][j]));
            }
        {
            // 4 KiB per wave in stage buffer 0 (every wave is past its last fragment read: barrier above): slab rows 256 B apart
            const unsigned tb = lds_offset(smem) + (unsigned)(wave * 4096);
            const unsigned wbase = tb + (unsigned)(r * 256);
            const unsigned rbase = tb + (unsigned)(g * 256);
            unsigned wad[4], rad[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wad[k] = wbase + (unsigned)((((4 * k + g) ^ r) & 15) << 4);               // row r, slot (4 j + g) ^ r
                rad[k] = rbase + (unsigned)(k * 1024) + (unsigned)(((r ^ (4 * k + g)) & 15) << 4);   // row 4 q + g, slot r ^ (4 q + g)
            }
            static_for<0, MI>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    lds_write16f(wad[j], acc[i][j]);
                });
                static_for<0, 4>([&](auto qc) {
                    constexpr int q = decltype(qc)::value;
                    lds_read16f<0>(acc[i][q], rad[q]);
                });
            });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(acc[i][q]));
        }
        if (a.ksplit > 1) {
            // split-K: the raw sums of this K range as plain rows of the partial buffer; the epilogue runs in the reduce kernel
            float* pb = a.part + blockIdx.y * a.part_stride + (n0 + 64 * wn + 4 * r);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m = m0 + WROWS * wm + g + 16 * i + 4 * q;
                    if (m < M) *reinterpret_cast<f32x4*>(pb + (long long)m * a.part_ld) = acc[i][q];
                }
            return;
        }
        atmvfi::plane_gemm_epilogue<CONVM, MI, BM, BN>(a, acc, cst, m0, n0, M, wm, wn, r, g);
    }
#ifdef ATMVFI_STAMP
    DUO_SUB(6);
    if (a.stamp && lane == 0) {
        unsigned long long* o = a.stamp + ((long long)blockIdx.x * 4 + wave) * 8;
        for (int k = 0; k < 7; ++k) o[k] = sub[k];
        o[7] = sub_t - t_begin;
    }
#endif
}

// Split-K, second half: the epilogue of the kernels above (gemm_common.h: output row of a GEMM row incl. the window-reverse map, row
// groups and the deconv's pixel shuffle; + bias, PReLU, + residual; fp32 rows and / or plane sink) on the sum of the partial buffers,
// added in split order: run-to-run deterministic.  One thread per (GEMM row, 4 columns).
__global__ __launch_bounds__(256) void gemm_splitk_reduce_kernel(const GemmDev a, int ngemm4) {
    fp16_saturate_on();
    const long long total = a.M * (long long)ngemm4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long m = idx / ngemm4;
        const int nb = (int)(idx - m * ngemm4) * 4;
        const atmvfi::ChanPos cp = atmvfi::gemm_chan_pos(a, nb);
        if (cp.nvalid <= 0) continue;
        // bias / slope of the four columns (selects, no indexed local arrays: hipcc turns those into scratch)
        auto vec4 = [&](const float* t, float dflt) -> f32x4 {
            if (!t) return (f32x4){dflt, dflt, dflt, dflt};
            if (cp.nvalid >= 4) return *reinterpret_cast<const f32x4*>(t + cp.co);
            f32x4 o = (f32x4){t[cp.co], dflt, dflt, dflt};
            if (cp.nvalid > 1) o.y = t[cp.co + 1];
            if (cp.nvalid > 2) o.z = t[cp.co + 2];
            return o;
        };
        const float* p = a.part + m * a.part_ld + nb;
        f32x4 v = *reinterpret_cast<const f32x4*>(p);
        for (int sp = 1; sp < a.ksplit; ++sp) v += *reinterpret_cast<const f32x4*>(p + sp * a.part_stride);
        float* orow;
        const float* rrow;
        long long prow;
        int pc0;
        if (!atmvfi::gemm_out_row(a, m, orow, rrow, prow, pc0)) continue;
        const f32x4 res = rrow ? atmvfi::gemm_load_residual4(rrow, cp) : (f32x4){0.f, 0.f, 0.f, 0.f};
        atmvfi::gemm_finish_store4(a, orow, prow, pc0, cp, v, vec4(a.bias, 0.f), vec4(a.prelu, 1.f), res);
    }
}

}  // namespace

template <bool CONVM, int BN, bool X3>
static int launch_duo(const GemmDev& d, int ngemm, hipStream_t s) {
    const size_t lds = (size_t)2 * stage_bytes(BN) + cst_floats(BN) * sizeof(float);
    const hipError_t attr_err = atmvfi::allow_dynamic_lds<gemm_duo_kernel<CONVM, BN, X3>>(lds);
    ATMVFI_REQUIRE(attr_err == hipSuccess, ATMVFI_ELAUNCH, "gemm_duo: hipFuncSetAttribute: %s", hipGetErrorString(attr_err));
    GemmDev dd = d;
    const int prc = atmvfi::plane_gemm_prepare("gemm_duo", dd, ngemm, BM, BN);
    if (prc != ATMVFI_OK) return prc;
#ifdef ATMVFI_STAMP
    dd.stamp = g_duo_stamp;
#endif
    if (dd.ksplit > 1) {
        hipLaunchKernelGGL((gemm_duo_kernel<CONVM, BN, X3>), dim3((unsigned)dd.vblocks, (unsigned)dd.ksplit), dim3(256), lds, s, dd);
        const int rc = atmvfi::check_launch("gemm_duo (split-K)");
        if (rc != ATMVFI_OK) return rc;
        const int ngemm4 = (ngemm + 3) / 4;
        const long long groups = d.M * ngemm4;
        hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3((unsigned)std::min<long long>((groups + 255) / 256, 8192)), dim3(256), 0, s, dd, ngemm4);
        return atmvfi::check_launch("gemm_duo (split-K reduce)");
    }
    hipLaunchKernelGGL((gemm_duo_kernel<CONVM, BN, X3>), dim3((unsigned)dd.vblocks), dim3(256), lds, s, dd);
    return atmvfi::check_launch("gemm_duo");
}

int atmvfi::launch_gemm_duo(const GemmDev& d, int ngemm, hipStream_t s) {
    // at most 64 GEMM columns: 64-column tiles (tile_wn = -2 forces the 128-column form for the A/B, -4 the 64-column one)
    const bool conv = d.mode == ATMVFI_GEMM_CONV;
    if ((ngemm <= 64 && d.force_wn != -2) || d.force_wn == -4) {
        if (d.terms == 1) return conv ? launch_duo<true, 64, false>(d, ngemm, s) : launch_duo<false, 64, false>(d, ngemm, s);
        return conv ? launch_duo<true, 64, true>(d, ngemm, s) : launch_duo<false, 64, true>(d, ngemm, s);
    }
    if (d.terms == 1) return conv ? launch_duo<true, 128, false>(d, ngemm, s) : launch_duo<false, 128, false>(d, ngemm, s);
    return conv ? launch_duo<true, 128, true>(d, ngemm, s) : launch_duo<false, 128, true>(d, ngemm, s);
}
