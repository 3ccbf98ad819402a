// LDS-DMA GEMM on split-plane activations, "ping-pong" schedule (gfx950): nn.Linear rows, ConvTranspose2d 2x2 / stride 2 and
// strided / dilated / 1x1 Conv2d (attention.py:138-141, 349-351, 93-96; network_base.py:20-32, 73-85, 417-424) whose input the
// producing layer left as split planes.
//
// Same arithmetic as gemm_split.hip / gemm_f16x3.hip (x = hi + lo'/1024 in fp16, three v_mfma_f32_16x16x32_f16 per product into two
// fp32 accumulators, k ascending, per accumulator the same order of products: bit-identical results), same operand layouts, same
// 256 x 128 tile on 512 threads (8 waves as 4 x 2, 64 x 64 each), same 48 KiB LDS stage x 3 filled by global_load_lds_dwordx4.
// What changes is WHEN things happen (the schedule conv3x3_planes.hip introduced for the 3x3 kernel):
//
//   * the eight waves form two groups (waves 0-3 / 4-7 = the two waves of each SIMD) that run ONE PHASE APART: while a group issues
//     the 48 MFMAs of k-step u from registers (s_setprio 1), its SIMD partners read the 16 fragments of their k-step from LDS
//     (ds_read_b128, one per-lane base + immediates) and issue their six DMA pieces of the stage two k-steps ahead; a raw
//     s_barrier swaps the roles.  gemm_split.hip interleaves fragment reads, DMA issue and MFMAs inside every wave and both waves
//     of a SIMD meet the same barrier in the same state: 2 400-2 700 cycles per k-step for 1 536 cycles of matrix work
//     (tools/stamp_split.py);
//   * waits: a wave's pieces of stage u+1 went out two read phases ago and six newer pieces (stage u+2) are allowed to stay in
//     flight (vmcnt(6)); the FIRST group waits at the end of its MFMA phase, the second at the end of its read phase -- the same
//     barrier -- so that stage u+1 is complete, for every wave, one barrier before its first reader (the first group) starts, and
//     both groups' pieces had 1.5-2 k-steps to land.  A stage's buffer is refilled one barrier after its last reader (the second
//     group) has drained its reads (lgkmcnt(0) before the barrier);
//   * the k-loop body has no data-dependent branch; the last two k-steps of a tile are separate copies: after the last tile they
//     issue nothing (nothing is in flight when the kernel ends), before that they put the next tile's constants and stages 0-1 in
//     flight -- the grid is PERSISTENT, one workgroup per CU walking its XCD's tiles, and the DMA ring flows across tiles;
//   * the epilogue is transposed through LDS (the wave's own DMA slots of the stage buffer that was read last), so that the 16 lanes
//     of an output row cover 256 contiguous bytes; both groups run it together (the first waits a phase for the second).  What follows
//     the transposition is gemm_plane.h's plane_gemm_epilogue, shared with gemm_duo.hip, as are the CONV-mode operand addressing
//     and the launcher's checks.
// Details and measurements at the places in the code and in DESIGN.md section 3.0b.
#include "gemm_plane.h"

#ifdef ATMVFI_STAMP
static unsigned long long* g_pp_stamp = nullptr;
extern "C" void atmvfi_debug_set_pp_stamp_buffer(void* p) { g_pp_stamp = (unsigned long long*)p; }
// per-k-step cycle sums (k-step index inside its tile, 0..15): 16 more values per wave behind the 8 of the phase stamps of every wave
#define PP_KSTAMP_BEGIN() unsigned long long kt0_ = 0; do { if (a.stamp) { __builtin_amdgcn_sched_barrier(0); kt0_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#define PP_KSTAMP_END(idx) do { if (a.stamp) { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) atomicAdd(&kst[wave * 16 + ((idx) < 15 ? (idx) : 15)], t_ - kt0_); __builtin_amdgcn_sched_barrier(0); } } while (0)
#define PP_STAMP(i) do { if (a.stamp) { tstamp[i] = __builtin_amdgcn_s_memtime(); rstamp[i] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#define PP_SUB(k) do { if (a.stamp) { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); sub[k] += t_ - sub_t; sub_t = t_; __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define PP_STAMP(i) do { } while (0)
#define PP_SUB(k) do { } while (0)
#define PP_KSTAMP_BEGIN() do { } while (0)
#define PP_KSTAMP_END(idx) do { } while (0)
#endif

namespace {

using atmvfi::GemmDev;

constexpr int BM = 256, BN = 128;
constexpr int STAGE = (2 * BM + 2 * BN) * 64;          // bytes: [A hi 256 rows][A lo][W hi 128 rows][W lo], 64 B per row
constexpr int A_LO = BM * 64, W_HI = 2 * BM * 64, W_LO = W_HI + BN * 64;
constexpr int PIECES = 6;                              // 16-byte DMA pieces per thread and stage: 4 of A, 2 of W
constexpr int CST_FLOATS = atmvfi::gemm_const_floats(BN) + BM;      // bias / slope of the column block + the tile's row-map entries

// X3: the three-term product (the default).  X3 == false (ATMVFI_PREC_F16): hi(x) * hi(w) alone -- no lo' fragment reads, 16 MFMAs per
// k-step instead of 48, no `cor`; DMA of both planes, stages, counted waits and barriers are the same source.
template <bool CONVM, bool X3>
__global__ __launch_bounds__(512, 2) void gemm_pp_kernel(const GemmDev a) {
    fp16_saturate_on();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int r = lane & 15;
    const int g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;

    // PERSISTENT GRID over an XCD-aware tile order.  Virtual block v: xcd = v & 7, slot = v >> 3, row tile = (slot / nblocks) * 8 + xcd,
    // column block = slot % nblocks (blocks v and v+8 share an XCD, so the column blocks of one row tile go to one L2).  Workgroup b
    // walks v = b, b + grid, ... (grid a multiple of 8: it stays on its XCD) and the DMA ring KEEPS FLOWING ACROSS TILES: the last two
    // k-steps of a tile put stages 0 and 1 of the workgroup's next tile in flight, so a tile's first DMA round trip (7-8 k cycles of
    // a 42 k-cycle K = 384 tile, tools/stamp_split.py) runs under the previous tile's last k-steps and epilogue.
    // (The launcher makes the grid persistent only for nk >= 2: the look-ahead of two stages then spans one tile boundary at most.)
    const int grid = gridDim.x;
    auto tile_of = [&](int v, int& tm0, int& tn0) {
        const int xcd = v & 7;
        const int slot = v >> 3;
        const int mgrp = slot / a.nblocks;
        const int nblk = slot - mgrp * a.nblocks;
        tm0 = (mgrp * 8 + xcd) * BM;
        tn0 = nblk * BN;
    };
    const int M = (int)a.M;                    // rows < 2^26 (launcher): 32-bit row arithmetic throughout
    int vb = blockIdx.x;
    int m0;
    int n0;
    tile_of(vb, m0, n0);
    if (m0 >= M) return;
    float* cst_base = reinterpret_cast<float*>(smem + 3 * STAGE);       // two buffers of per-tile constants

    // ---- DMA pieces of this wave.  A: rows (i * 8 + wave) * 16 + lane / 4 (i = 0, 1) of the hi and of the lo plane; W: rows
    // wave * 16 + lane / 4 of both planes.  The LDS image of a piece is wave-uniform base + lane * 16 B; the 16-byte slot swizzle
    // goes on the SOURCE address.  Per lane: three 32-bit byte offsets from wave-uniform plane pointers that advance by one
    // 32-channel chunk (A: in_ld rows, W: wrows rows) per k-step.  They belong to the ISSUER's tile: the tile whose stages are being
    // put in flight -- the tile of the MFMAs or, in its last two k-steps, the next one.
    const unsigned ls16 = (unsigned)(((lane & 3) ^ swz64(lane >> 2)) << 4);       // swz64(16 k + row) == swz64(row)
    unsigned aoff[2];
    unsigned wsoff;
    const unsigned char* pa_hi;
    const unsigned char* pa_lo;
    const unsigned char* pw_hi;
    const unsigned char* pw_lo;
    // CONV mode (gemm_plane.h): per lane and row the input row of tap (0, 0) and its (y, x); wave-uniform the tap and chunk of the stage
    // that goes out next (aoff is not used)
    atmvfi::PlaneConvWalk cv;
    const int zero_row = a.in_N * a.H * a.W;
    auto setup_issue = [&](int tm0, int tn0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int m = tm0 + (i * 8 + wave) * 16 + (lane >> 2);
            if (m >= M) m = M - 1;                                  // tail rows: valid address, result never stored
            if constexpr (CONVM) atmvfi::plane_conv_row<true>(a, m, i, cv);         // (divisors laundered: the kernel is at the register limit)
            else aoff[i] = (unsigned)m * 64u + ls16;
        }
        int n = tn0 + wave * 16 + (lane >> 2);
        if (n >= a.wrows) n = a.wrows - 1;                          // columns past the packed rows: never stored
        wsoff = (unsigned)n * 64u + ls16;
        pa_hi = reinterpret_cast<const unsigned char*>(a.a_hi);
        pa_lo = reinterpret_cast<const unsigned char*>(a.a_lo);
        pw_hi = reinterpret_cast<const unsigned char*>(a.w_hi);
        pw_lo = reinterpret_cast<const unsigned char*>(a.w_lo);
        cv.ky = cv.kx = cv.chunk = 0;
    };
    setup_issue(m0, n0);
    const long long a_step = (long long)a.in_ld * 64, w_step = (long long)a.wrows * 64;
    int wr_off = 0;                                                 // stage buffer (byte offset) the next issue goes to
    auto issue_stage = [&]() {
        unsigned char* dst = smem + wr_off + wave * 1024;
        if constexpr (CONVM) {
            atmvfi::plane_conv_issue<A_LO, 8 * 1024>(a, cv, pa_hi, pa_lo, a_step, zero_row, ls16, dst);
        } else {
            dma16(pa_hi + aoff[0], dst);
            dma16(pa_hi + aoff[1], dst + 8 * 1024);
            dma16(pa_lo + aoff[0], dst + A_LO);
            dma16(pa_lo + aoff[1], dst + A_LO + 8 * 1024);
            pa_hi += a_step;
            pa_lo += a_step;
        }
        dma16(pw_hi + wsoff, dst + W_HI);
        dma16(pw_lo + wsoff, dst + W_LO);
        pw_hi += w_step;
        pw_lo += w_step;
        wr_off = wr_off == 2 * STAGE ? 0 : wr_off + STAGE;
    };
    // Per-tile constants by LDS-DMA, two pieces per wave: bias / slope of the column block, and the tile's BM row-map entries (LINEAR
    // with an out_row_map: the window-reverse scatter of proj; a global load of the map in the epilogue would cost a memory latency
    // per tile).  Without a map the second piece repeats the first (same bytes, same place): the counted waits stay uniform.
    auto dma_tile_consts = [&](int tm0, int tn0, float* dst) {
        atmvfi::gemm_dma_consts<BN>(a, tn0, dst, wave, lane);
        if (a.out_row_map && a.mode == ATMVFI_GEMM_LINEAR) {
            int m = tm0 + (wave & 3) * 64 + lane;
            if (m >= M) m = M - 1;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.out_row_map + m),
                                             (__attribute__((address_space(3))) void*)(dst + atmvfi::gemm_const_floats(BN) + (wave & 3) * 64), 4, 0, 0);
        } else {
            atmvfi::gemm_dma_consts<BN>(a, tn0, dst, wave, lane);
        }
    };

    f32x4 acc[4][4];
    RegsIf<X3, f32x4[4][4]> cor;

#ifdef ATMVFI_STAMP
    unsigned long long* kst = reinterpret_cast<unsigned long long*>(smem + 3 * STAGE + 2 * CST_FLOATS * sizeof(float));
    if (tid < 128) kst[tid] = 0;
    __syncthreads();
    unsigned long long tstamp[4], rstamp[4];
    unsigned long long t_loop = 0, t_epi = 0, r_loop = 0, r_epi = 0, t_pro = 0, r_pro = 0;
    int ntile = 0;
    unsigned long long sub[3] = {0, 0, 0}, sub_t = 0;
#endif
    PP_STAMP(0);
    const int nk = a.nchunks32;
    // ---- prologue of the first tile: constants, stages 0 and 1
    dma_tile_consts(m0, n0, cst_base);
    issue_stage();
    if (nk > 1) {
        issue_stage();
        wait_vm<PIECES>();
    } else {
        wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();          // the second group runs one phase behind

    f16x8 xh[4], wh[4];
    RegsIf<X3, f16x8[4]> xl, wl;
    const unsigned xfrag = lds_offset(smem) + (unsigned)((64 * wm + r) * 64 + ((g ^ swz64(r)) << 4));
    const unsigned wfrag = lds_offset(smem) + (unsigned)(W_HI + (64 * wn + r) * 64 + ((g ^ swz64(r)) << 4));
    int rd_off = 0;                                      // stage buffer (byte offset) of the k-step being read
    int seq = 0;                                         // tiles done by this workgroup
    // this workgroup's next tile (row tiles only grow along a workgroup's walk: the first empty one ends it)
    int nm0 = 0;
    int nn0 = 0;
    bool has_next = false;

    // One k-step of one wave.  KIND 0: a k-step with two more k-steps of its tile behind it -- the stage two k-steps ahead goes out,
    // six pieces stay in flight at the wait.  KIND 1: the tile's last k-step but one -- the ring moves on to the next tile (its
    // constants and stage 0; eight pieces in flight), or nothing goes out (wait for everything).  KIND 2: the last k-step --
    // stage 1 of the next tile, or nothing (and no wait: there is no next stage).  g1wait: false in the first k-step of a later
    // tile for the second group, which waited before its epilogue (its stores would otherwise sit in front of the counted wait).
    auto kstep = [&](auto kind_c, bool g1wait) {
        constexpr int KIND = decltype(kind_c)::value;
        // ---------------- read phase ----------------
        const unsigned xa = xfrag + (unsigned)rd_off, wa = wfrag + (unsigned)rd_off;
        static_for<0, 4>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            lds_read16<i * 1024>(xh[i], xa);
            if constexpr (X3) lds_read16<i * 1024 + A_LO>(xl[i], xa);
        });
        static_for<0, 4>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            lds_read16<j * 1024>(wh[j], wa);
            if constexpr (X3) lds_read16<j * 1024 + BN * 64>(wl[j], wa);
        });
        rd_off = rd_off == 2 * STAGE ? 0 : rd_off + STAGE;
        if constexpr (KIND == 0) {
            issue_stage();
        } else if constexpr (KIND == 1) {
            if (has_next) {
                setup_issue(nm0, nn0);
                dma_tile_consts(nm0, nn0, cst_base + ((seq + 1) & 1) * CST_FLOATS);
                issue_stage();
            }
        } else {
            if (has_next) issue_stage();
        }
        auto wait_next = [&]() {
            if constexpr (KIND == 0) {
                wait_vm<PIECES>();
            } else if constexpr (KIND == 1) {
                if (has_next) wait_vm<PIECES + 2>();
                else wait_vm<0>();
            } else {
                if (has_next) wait_vm<PIECES>();
            }
        };
        if (grp == 1 && g1wait) wait_next();
        if constexpr (X3) {
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(xh[0]), "+v"(xh[1]), "+v"(xh[2]), "+v"(xh[3]), "+v"(xl[0]), "+v"(xl[1]), "+v"(xl[2]), "+v"(xl[3]));
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(wh[j]), "+v"(wl[j]));
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(xh[0]), "+v"(xh[1]), "+v"(xh[2]), "+v"(xh[3]));
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(wh[j]));
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---------------- MFMA phase ----------------
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (X3) cor[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j], xh[i], cor[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xh[i], acc[i][j], 0, 0, 0);
            }
        if constexpr (X3) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) cor[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xl[i], cor[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        if (grp == 0) wait_next();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };

    for (;;) {
        const int nxt = vb + grid;
        has_next = false;
        if (nxt < a.vblocks) {
            tile_of(nxt, nm0, nn0);
            has_next = nm0 < M;
        }
        const float* cst = cst_base + (seq & 1) * CST_FLOATS;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                // pinned: hipcc otherwise folds the zeros into the first MFMAs' C operand and uses the (then dead) accumulator
                // registers as temporaries of the first read phase, guarded by s_waitcnt vmcnt(0)
                if constexpr (X3) {
                    cor[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    asm volatile("" : "+v"(acc[i][j]), "+v"(cor[i][j]));
                } else {
                    asm volatile("" : "+v"(acc[i][j]));
                }
            }
        PP_STAMP(1);
        {
            bool g1wait = seq == 0;
            for (int kc = 0; kc + 2 < nk; ++kc) {
                PP_KSTAMP_BEGIN();
                kstep(std::integral_constant<int, 0>{}, g1wait);
                PP_KSTAMP_END(kc);
                g1wait = true;
            }
            if (nk >= 2) {
                PP_KSTAMP_BEGIN();
                kstep(std::integral_constant<int, 1>{}, g1wait);
                PP_KSTAMP_END(nk - 2);
                g1wait = true;
            }
            {
                PP_KSTAMP_BEGIN();
                kstep(std::integral_constant<int, 2>{}, g1wait);
                PP_KSTAMP_END(nk - 1);
            }
        }
        PP_STAMP(2);
#ifdef ATMVFI_STAMP
        sub_t = __builtin_amdgcn_s_memtime();
#endif
        // Both groups run the epilogue AT THE SAME TIME: the first group waits here for the second one's last MFMA phase (one phase,
        // ~900 cycles), and two epilogue waves per SIMD fill each other's VALU latencies.  (One group's epilogue beside the other
        // group's last MFMA phase / first read phase of the next tile, i.e. one after the other, cost 15 k cycles per tile boundary
        // against 22 k of k-loop at K = 384: a lone epilogue wave per SIMD runs its dependent VALU chains at ~7 cycles an instruction.)
        if (grp == 0) __builtin_amdgcn_s_barrier();
        // The second group's pieces of the next tile's stage 1 (all that is in flight) are waited for HERE, before its stores join
        // the queue; its first k-step of the next tile then skips the counted wait (g1wait).
        if (grp == 1 && has_next) wait_vm<0>();

        // ---- epilogue (gemm_plane.h: why and how the slabs are transposed, and everything behind the transposition).  The 4 KiB a wave
        // needs are ITS OWN four A pieces of the stage buffer the last k-step was read from: nobody reads that buffer any more (this
        // group's epilogue starts a barrier after the other group's last read), and the only DMA that can land there before this wave
        // is done is the wave's own next issue.  Slot XOR-swizzle (physical slot = slot ^ row): conflict-free for the 8-lane
        // groups of ds_write_b128 (banks mod 32) and the 16-lane groups of ds_read_b128 (MI355X_MICROARCH.md, LDS).
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (X3) acc[i][j] = acc[i][j] + cor[i][j] * LO_UNSCALE;
                asm volatile("" : "+v"(acc[i][j]));
            }
        {
            const unsigned xb = (unsigned)(rd_off == 0 ? 2 * STAGE : rd_off - STAGE);          // buffer of the last k-step
            const unsigned tb = lds_offset(smem) + xb + (unsigned)(wave * 1024);
            const unsigned wbase = tb + (unsigned)((r >> 2) * 8192 + (r & 3) * 256 + ((g ^ (r & 3)) << 4));
            const unsigned rq6 = (unsigned)((r >> 2) << 6);
            const unsigned rbase = tb + (unsigned)(g * 256);
            const unsigned rg4 = (unsigned)((r ^ g) << 4);
            unsigned wad[4], rad[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wad[k] = wbase + (rq6 ^ (unsigned)(k << 6));                    // slot (4 j + g) ^ r of row r
                rad[k] = rbase + (rg4 ^ (unsigned)(k << 6));                    // slot r ^ (4 q + g) of row 4 q + g (+ q * 8192 below)
            }
            static_for<0, 4>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                static_for<0, 4>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    lds_write16f(wad[j], acc[i][j]);
                });
                static_for<0, 4>([&](auto qc) {
                    constexpr int q = decltype(qc)::value;
                    lds_read16f<q * 8192>(acc[i][q], rad[q]);
                });
            });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(acc[i][q]));
        }
        PP_SUB(0);
        atmvfi::plane_gemm_epilogue<CONVM, 4, BM, BN>(a, acc, cst, m0, n0, M, wm, wn, r, g, [&] { PP_SUB(1); });
        PP_SUB(2);
        PP_STAMP(3);
#ifdef ATMVFI_STAMP
        if (a.stamp) {
            if (seq == 0) { t_pro = tstamp[1] - tstamp[0]; r_pro = rstamp[1] - rstamp[0]; }
            t_loop += tstamp[2] - tstamp[1]; r_loop += rstamp[2] - rstamp[1];
            t_epi += tstamp[3] - tstamp[2]; r_epi += rstamp[3] - rstamp[2];
            ++ntile;
        }
#endif
        if (!has_next) break;
        if (grp == 1) __builtin_amdgcn_s_barrier();          // the second group drops one phase behind again
        vb = nxt;
        m0 = nm0;
        n0 = nn0;
        ++seq;
    }
#ifdef ATMVFI_STAMP
    if (a.stamp && lane == 0) {
        unsigned long long* o = a.stamp + ((long long)blockIdx.x * 8 + wave) * 8;
        o[0] = t_pro; o[1] = t_loop / ntile; o[2] = t_epi / ntile;
        o[3] = (unsigned long long)nk;
        o[4] = r_loop / ntile; o[5] = sub[0] / ntile; o[6] = sub[1] / ntile;
        o[7] = sub[2] / ntile;
    }
    __syncthreads();
    if (a.stamp && tid < 128) a.stamp[(long long)gridDim.x * 64 + (long long)blockIdx.x * 128 + tid] = kst[tid] / (ntile ? ntile : 1);
#endif
}

}  // namespace

template <bool CONVM, bool X3>
static int launch_pp(const GemmDev& d, int ngemm, hipStream_t s) {
#ifdef ATMVFI_STAMP
    const size_t lds = (size_t)3 * STAGE + 2 * CST_FLOATS * sizeof(float) + 1024;      // + the per-k-step stamp sums
#else
    const size_t lds = (size_t)3 * STAGE + 2 * CST_FLOATS * sizeof(float);
#endif
    const hipError_t attr_err = atmvfi::allow_dynamic_lds<gemm_pp_kernel<CONVM, X3>>(lds);
    ATMVFI_REQUIRE(attr_err == hipSuccess, ATMVFI_ELAUNCH, "gemm_pp: hipFuncSetAttribute: %s", hipGetErrorString(attr_err));
    GemmDev dd = d;
    const int rc = atmvfi::plane_gemm_prepare("gemm_pp", dd, ngemm, BM, BN);
    if (rc != ATMVFI_OK) return rc;
#ifdef ATMVFI_STAMP
    dd.stamp = g_pp_stamp;
#endif
    // persistent from two k-steps up (the ring's look-ahead of two stages then spans at most one tile boundary): one workgroup per
    // CU (147 KiB of LDS) walking its XCD's tiles; K <= 32: one workgroup per tile
    const int grid = d.nchunks32 >= 2 ? std::min(dd.vblocks, atmvfi::cu_count()) : dd.vblocks;
    hipLaunchKernelGGL((gemm_pp_kernel<CONVM, X3>), dim3((unsigned)grid), dim3(512), lds, s, dd);
    return atmvfi::check_launch("gemm_pp");
}

int atmvfi::launch_gemm_pp(const GemmDev& d, int ngemm, hipStream_t s) {
    if (d.terms == 1) return d.mode == ATMVFI_GEMM_CONV ? launch_pp<true, false>(d, ngemm, s) : launch_pp<false, false>(d, ngemm, s);
    return d.mode == ATMVFI_GEMM_CONV ? launch_pp<true, true>(d, ngemm, s) : launch_pp<false, true>(d, ngemm, s);
}
