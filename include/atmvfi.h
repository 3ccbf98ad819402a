/*
 * atmvfi.h -- C ABI of libatmvfi_hip.so: the MI355X (gfx950) kernels underneath the
 * ATM-VFI `Network.forward` hot path.
 *
 * The reference (Gancheekim/ATM-VFI) has no FFI seam: every device op is an implicit
 * ATen call issued from Python.  Each entry point below therefore
 * cites the reference *call site(s)* whose arithmetic it replaces.  The Python host
 * (atm-vfi_amd/hip_ops.py) binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless stated; the library allocates
 *    nothing, owns nothing and keeps no mutable global state (re-entrant per stream; the only caches are per-device
 *    constants: CU count and "dynamic LDS limit already raised for this kernel"); it reads no environment variable -- the
 *    diagnostic builds (`make stamp`, `make ablate`) do, and are never loaded by the product;
 *  - `stream` is a hipStream_t passed as void* (0 = default stream);
 *  - feature maps are NHWC "views": (ptr, ld) with ptr already advanced to the first
 *    channel of the view and `ld` = floats between consecutive pixels.  Views let a
 *    producer write straight into a slice of a wider concat buffer, so torch.cat /
 *    einops.rearrange of the reference never materialise.  ld % 4 == 0 and 16-byte
 *    aligned pointers are required (checked; ATMVFI_EALIGN);
 *  - image-like tensors (3-channel frames, 2-channel flows, 1-channel masks) are
 *    planar NCHW, exactly as the reference's API returns them;
 *  - return value: 0 on success, negative ATMVFI_E* otherwise; atmvfi_last_error()
 *    gives a thread-local message.  Shapes are validated on the host BEFORE launch.
 */
#ifndef ATMVFI_H
#define ATMVFI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATMVFI_OK        0
#define ATMVFI_EINVAL   -1   /* bad shape / null pointer / unsupported configuration */
#define ATMVFI_EALIGN   -2   /* pointer or leading dimension not 16-byte aligned */
#define ATMVFI_ELAUNCH  -3   /* HIP launch error */

int         atmvfi_version(void);            /* (major<<16)|(minor<<8)|patch */
const char* atmvfi_last_error(void);
/* sha256 (hex) over the sources this library was built from (tools/source_digest.py: atm-vfi_amd/csrc/{*.hip,*.h,*.inc,Makefile} +
 * this header), baked in at build time: lets a caller prove that a shipped .so belongs to the shipped sources.  The reference has
 * no counterpart (pure Python, nothing is built). */
const char* atmvfi_source_digest(void);
/* The f16x3 engines' operand range contract at run time.  Contraction operands are split as x = hi + lo'/1024 in fp16: |x| beyond
 * 65504 saturates silently (finite, but no longer what the fp32 reference computes).  The CHECKED build of this library
 * (libatmvfi_hip_checked.so: the same sources with -DATMVFI_RANGE_CHECK, `make checked`) counts, in a device word the caller
 * attaches, every pair of activations whose split produced a hi half at the fp16 limit or non-finite (|x| > 65488, inf, NaN) --
 * at every place an activation is split: the plane sinks of all producers and the in-kernel operand splits.  `word`: a zeroed
 * device uint32 that must outlive the launches (NULL detaches); attached for the CURRENT device, ordered on `stream`.
 * atmvfi_range_checked(): 1 in the checked build, 0 in the default one, where atmvfi_range_word_set fails with ATMVFI_EINVAL
 * and no kernel carries an extra instruction.  The reference has no counterpart (it computes in fp32). */
int atmvfi_range_word_set(uint32_t* word, void* stream);
int atmvfi_range_checked(void);

/* ------------------------------------------------------------------------------------
 * Implicit-GEMM contraction engine on fp32 MFMA (v_mfma_f32_16x16x4_f32).
 *
 * One kernel family serves the three contraction shapes of the hot path:
 *   ATMVFI_GEMM_CONV   Conv2d k in {1,3}, stride {1,2,4}, dilation {1,2}, zero pad
 *                      (network_base.py:20-25 conv(); :42-48 fusion convs; :158,:195 heads)
 *   ATMVFI_GEMM_LINEAR nn.Linear over token rows (attention.py:138-141,349-351 q/kv/qkv/proj;
 *                      :93-96 fc1/fc2), with optional row groups / row scatter map
 *   ATMVFI_GEMM_DECONV ConvTranspose2d(k2,s2,p0) (network_base.py:27-32 deconv()) as a GEMM to
 *                      4*Cout columns with a pixel-shuffle store
 * Epilogue, in order: + bias[co]; PReLU(slope[co]) if `prelu`; + residual if `residual`.
 * `in_prelu` applies a per-input-channel PReLU while loading the input (the leading
 * nn.PReLU of upsample_pyramid stages 1-2, network_base.py:209,215).
 * ---------------------------------------------------------------------------------- */
#define ATMVFI_GEMM_CONV   0
#define ATMVFI_GEMM_LINEAR 1
#define ATMVFI_GEMM_DECONV 2

typedef struct atmvfi_gemm_params {
    int32_t mode;
    /* input view.  CONV/DECONV: NHWC [N,H,W,Cin].  LINEAR: rows; row m lives at
       in + (m / in_rpg) * in_gstride + (m % in_rpg) * in_ld   (in_rpg == 0: m * in_ld) */
    const float* in;
    int32_t in_ld, N, H, W, Cin;
    int64_t in_gstride; int32_t in_rpg;
    /* weights packed by atmvfi_pack_*: [Nrows16][taps][CinPad16] fp32, zero padded */
    const float* weight;
    int32_t Cout, kh, kw, stride, pad, dil;
    int32_t Ho, Wo;            /* CONV: output size; DECONV: 2H,2W; LINEAR: ignored */
    int64_t M;                 /* LINEAR: number of rows; others: N*Ho*Wo (CONV) / N*H*W (DECONV) */
    /* output view; row r at out + (r / out_rpg) * out_gstride + (r % out_rpg) * out_ld */
    float* out;
    int32_t out_ld;
    int64_t out_gstride; int32_t out_rpg;
    const int32_t* out_row_map;   /* optional [M]: destination row per GEMM row, <0 = drop */
    const float* bias;            /* [Cout] or NULL */
    const float* prelu;           /* [Cout] or NULL */
    const float* in_prelu;        /* [Cin]  or NULL */
    const float* residual;        /* optional, indexed by GEMM row m (before out_row_map) */
    int32_t res_ld;
    /* ATMVFI_PREC_F32: exact fp32 MFMA on `weight`.  ATMVFI_PREC_F16X3: split-precision engine
       (x = hi + lo'/1024 in fp16, three 16-bit MFMAs per product, fp32 accumulate) on the two
       fp16 planes written by atmvfi_pack_weight_split; in_prelu must then be padded to 32. */
    int32_t precision;
    const void* weight_hi;
    const void* weight_lo;
    /* Split-plane input (F16X3; every mode, CONV: see in_hi2 below): when in_hi/in_lo are set the activations are read by LDS-DMA from two
       fp16 planes in the chunk-major layout [Cin/32 chunks][plane rows][32] written by a producer kernel's sink or by
       atmvfi_split_planes; `in_ld` is then the plane row count (>= M), `in` is ignored, the pad channels of the last chunk must be
       finite (they meet zero weights). */
    const void* in_hi;
    const void* in_lo;
    /* Plane sink (F16X3 only): when out_hi/out_lo are set the result is written (also, or -- with out == NULL -- only) as split
       planes in the same chunk-major layout with out_plane_rows rows per chunk: channel co of output row r goes to plane row
       r % out_rpg, channel out_plane_c0 + (r / out_rpg) * out_plane_gc + co (out_rpg == 0: row r, channel out_plane_c0 + co;
       DECONV: r = output pixel n*Ho*Wo + y*Wo + x; with out_row_map, r is the mapped row).  Channel offsets are multiples of 4;
       channels past Cout inside the last group of 4 are written as zero.  This is the input format of atmvfi_conv3p
       and of atmvfi_gemm's in_hi/in_lo: consecutive contraction layers hand activations over without an fp32 copy. */
    void* out_hi;
    void* out_lo;
    int64_t out_plane_rows;
    int32_t out_plane_c0, out_plane_gc;
    /* F16X3, fp32 input: n-tiles of 16 columns per 256-row workgroup tile, 0 = cost model (default), 1..8 = forced (sweeps).
       F16X3, split-plane input: 0 = chosen per launch between the ping-pong kernel (gemm_pp.hip: 256 x 128 tiles, persistent grid) and
       gemm_duo.hip (128 x 128 tiles, two workgroups per CU: grids that would leave half of the CUs idle; 128 x 64 tiles for layers of
       at most 64 columns); -3 forces gemm_pp.hip, -2 / -4 gemm_duo.hip with 128- / 64-column tiles, -1 the reference schedule
       (gemm_split.hip).  All have the same arithmetic: bit-identical results (parity tests, same-process A/B). */
    int32_t tile_wn;
    /* CONV mode on split-plane input (in_hi / in_lo): rows are input pixels n*H*W + y*W + x, in_ld > N*H*W and row N*H*W of every chunk
       is zero (taps outside the image read it).  Optionally the input channels come from TWO plane buffers (a torch.cat of the
       reference that never materialises): chunks 0 .. in_split_chunks-1 from in_hi / in_lo, the rest from in_hi2 / in_lo2 (in_ld2 rows
       per chunk, same pixel rows, same zero-row contract); both parts are whole 32-channel chunks. */
    const void* in_hi2;
    const void* in_lo2;
    int32_t in_ld2, in_split_chunks;
    /* Split-K scratch (F16X3, split-plane input; optional): with `workspace` (fp32, 16-byte aligned) of at least
       atmvfi_gemm_workspace_floats(M, ngemm, k-steps) floats the launcher may cut a long K of an under-filled grid (small frames:
       a few tiles walking 40-150 k-steps on a mostly idle chip) into up to 8 ranges of k-steps, one workgroup per (tile, range)
       writing raw fp32 partial sums, and a second kernel that adds them IN RANGE ORDER and runs the epilogue.  Run-to-run
       deterministic; differs from the unsplit launch by fp32 summation order only.  NULL: never split. */
    float* workspace;
    int64_t workspace_floats;
} atmvfi_gemm_params;

#define ATMVFI_PREC_F32   0
#define ATMVFI_PREC_F16X3 1
/* Single-pass fp16 (opt-in; never a default): a product is hi(x) * hi(w) alone -- hi = the split's high half, fp16 round-to-nearest-even,
   saturating -- accumulated in fp32 in the engine's k order into one accumulator: one v_mfma_f32_16x16x32_f16 per product instead of
   three, about 11 significand bits per operand.  Accepted ONLY with split-plane input (in_hi and in_lo set), on the gemm_pp / gemm_duo
   engines: tile_wn 0 (auto, split-K included), -2, -3, -4.  With fp32 input, or with tile_wn = -1 (the reference schedule has no such
   instance), the call returns ATMVFI_EINVAL before any launch.  Weights (weight_hi / weight_lo, both required: the layouts do not
   change) and the plane sink follow the rules of ATMVFI_PREC_F16X3; a sink still writes BOTH planes, the exact split of the launch's own
   fp32 result.  The tile and split-K choices do not depend on the precision.  The reference has no counterpart (it computes in fp32). */
#define ATMVFI_PREC_F16   2

int atmvfi_gemm(const atmvfi_gemm_params* p, void* stream);
/* fp32 elements of split-K scratch the plane-input GEMM wants for M rows, ngemm GEMM columns (Cout; 4 * round_up(Cout, 4) for DECONV)
 * and ksteps = taps * ceil(Cin / 32) k-steps on this device; 0: it would not split that shape. */
int64_t atmvfi_gemm_workspace_floats(int64_t M, int ngemm, int ksteps);

/* 1x1 convolution with 1 <= Cout <= 8 output channels on split-plane input: the read-out nn.Conv2d(hidden, 5, 1) of the motion MLPs
 * (network_base.py:158,195 local_motion_mlp[2] / global_motion_mlp[2]).  in_hi / in_lo: chunk-major planes of `rows` pixel rows
 * (plane_rows rows per 32-channel chunk); weight: the layer's fp32 [Cout][Cin] (the nn.Conv2d weight as it is); out: fp32 rows,
 * out_ld floats apart, Cout written per row.  fp32 FMAs on x = hi + lo'/1024. */
int atmvfi_head1x1_planes(const void* in_hi, const void* in_lo, int64_t plane_rows, int64_t rows, int Cin, const float* weight,
                          const float* bias, int Cout, float* out, int out_ld, void* stream);

/* fp32 rows [M, C] (row stride in_ld floats) -> the two fp16 planes of the split-plane format, hi = fp16(x),
   lo = fp16((x - hi) * 1024), both saturating, chunk major: element (row, c) at ((c / 32) * plane_rows + row) * 32 + c % 32
   (each plane holds ceil(C / 32) * plane_rows * 32 halves; the pad channels of the last chunk are written as zero).
   `prelu` (optional, [C]) is applied to the values first. */
int atmvfi_split_planes(const float* in, int in_ld, int64_t M, int C, const float* prelu, void* hi, void* lo, int plane_rows, void* stream);
/* The same into a channel range of wider planes: the C channels go to plane channels c0 .. c0 + C (c0 a multiple of 8), channels up to
   the next multiple of pad_to (8, or 32 with c0 a multiple of 32) are written as zero, everything else is left alone. */
int atmvfi_split_planes_at(const float* in, int in_ld, int64_t M, int C, const float* prelu, void* hi, void* lo, int plane_rows, int c0,
                           int pad_to, void* stream);

/* Convenience wrappers with the reference-layer names (thin shims over atmvfi_gemm). */
int atmvfi_conv2d(const atmvfi_gemm_params* p, void* stream);
int atmvfi_linear(const atmvfi_gemm_params* p, void* stream);
int atmvfi_deconv2x2(const atmvfi_gemm_params* p, void* stream);

/* Weight re-layout (device -> device, run once per checkpoint load).
 *  conv  : OIHW [Cout,Cin,kh,kw]  -> [rows16(Cout)][kh*kw][CinPad16]
 *  linear: [Cout,Cin]             -> same with one tap
 *  deconv: IOHW [Cin,Cout,2,2]    -> [rows16(4*CoutP4)][1][CinPad16], row = (a*2+b)*CoutP4 + co
 * `dst` must hold atmvfi_packed_weight_floats(...) floats. */
int64_t atmvfi_packed_weight_floats(int mode, int Cout, int Cin, int kh, int kw);
int atmvfi_pack_weight(int mode, const float* src, float* dst, int Cout, int Cin, int kh, int kw, void* stream);

/* ------------------------------------------------------------------------------------
 * Split-precision ("f16x3") 3x3 / stride 1 / pad 1 convolution -- the same Conv2d(+PReLU) call
 * sites as ATMVFI_GEMM_CONV (network_base.py:20-25), two thirds of the network's FLOPs.
 * Every fp32 operand is split as x = hi + lo (fp16 each) and hi*hi + hi*lo + lo*hi is accumulated
 * in fp32 on v_mfma_f32_16x16x32_f16 (3 MFMAs at 16x the fp32-MFMA rate; ~22 significand bits,
 * finite for |x| < 1.3e5).  The input halo of a 16x16 output tile is staged in LDS once per
 * 32-channel chunk and reused by all nine taps.  Epilogue: + bias[co]; PReLU(slope[co]).
 * Split weights of the two GEMM engines (atmvfi_gemm with precision F16X3): atmvfi_pack_weight_split writes two fp16 planes
 * (atmvfi_split_weight_halves() halves each), K-STEP MAJOR: [k-step = tap * CinPad32/32 + chunk][row16][32 halves], same source
 * layouts and row order as atmvfi_pack_weight -- the 16 rows x 64 bytes one load / LDS-DMA instruction moves are one contiguous KiB.
 * ---------------------------------------------------------------------------------- */
int64_t atmvfi_split_weight_halves(int mode, int Cout, int Cin, int kh, int kw);
int atmvfi_pack_weight_split(int mode, const float* src, void* dst_hi, void* dst_lo, int Cout, int Cin, int kh, int kw,
                             void* stream);
/* Weights of atmvfi_conv3x3_f16x3 (OIHW [Cout,Cin,3,3] -> two fp16 planes of atmvfi_conv3x3_weight_halves halves each), k-step
 * major: [k-step][row padded to 16][32 halves], k-step = (32-channel chunk, tap); when 1 <= Cin % 32 <= 8 the channel tail is
 * tap-packed into three more k-steps of 4 taps x 8 channels, so that e.g. the 32k+5-wide decoder maps do not pay nine 32-wide
 * k-steps for five channels.  Layout details: csrc/conv3x3_f16x3.hip. */
int64_t atmvfi_conv3x3_weight_halves(int Cout, int Cin);
int atmvfi_pack_weight_conv3x3(const float* src, void* dst_hi, void* dst_lo, int Cout, int Cin, void* stream);
/* Optional second output (out_hi / out_lo non-null): the result once more as split planes -- fp16 hi and lo' = (x - hi) * 1024,
 * chunk major [ceil(Cout/32)][plane_rows][32] with pixel n*H*W + y*W + x as the row, see atmvfi_split_planes -- after a
 * per-channel PReLU of its own (plane_prelu, padded to a multiple of 32 floats, or null).  That is the operand format of the
 * LDS-DMA GEMM behind atmvfi_deconv2x2 / atmvfi_linear (in_hi / in_lo): the decoder's conv -> PReLU -> ConvTranspose2d chain
 * (network_base.py:207-216) hands over without a separate split pass.  Pad channels of the last chunk must be zero in the
 * caller's buffer; those inside the last group of 4 are written as zero. */
int atmvfi_conv3x3_f16x3(const float* in, int in_ld, int N, int H, int W, int Cin, const void* w_hi, const void* w_lo,
                         int Cout, float* out, int out_ld, const float* bias, const float* prelu, void* out_hi, void* out_lo,
                         int64_t plane_rows, const float* plane_prelu, int schedule, int wn, void* stream);
/* schedule / wn: the kernel has two schedules (512-thread 16x16 tiles, one workgroup per CU; 256-thread 16x8 tiles, two per CU) and
 * 1..8 n-tiles of 16 output channels per workgroup, picked per layer from a cost model.  Per call: schedule -1 = cost model,
 * 0 = row, 1 = half; wn 0 = cost model, 1..8 = n-tiles per workgroup (parity tests reach every instance this way; results do not
 * depend on either).  The library keeps no process-wide override. */
/* The same convolution on SPLIT-PLANE input (csrc/conv3x3_planes.hip), as ONE call on a parameter block: the activations are the two
 * fp16 planes (hi, lo', chunk major [ceil(Cin/32)][in_rows][32], row = pixel n*H*W + y*W + x) that the producing layer's sink wrote, so
 * the input halo goes global -> LDS by LDS-DMA with no register staging and no conversion, and the two waves of each SIMD run one phase
 * apart (one issues MFMAs while the other reads fragments and issues DMA).  Bit-identical to atmvfi_conv3x3_f16x3 on the same values.
 * A zeroed block plus in_hi / in_lo / in_rows, N / H / W / Cin, w_hi / w_lo / Cout, one output and terms is the plain convolution; fields
 * are only ever appended and zero means off (as atmvfi_gemm_params), so a block of an older caller keeps its meaning.
 *  - Input planes.  in_rows > N*H*W and row N*H*W of every chunk is ZERO (it is the source of the halo pixels that fall outside the
 *    image; atm-vfi_amd's Planes.alloc reserves it); pad channels of the last chunk are zero; in_rows * 64 < 2^32.
 *  - fp32 output (may be NULL).  `out` is the ADDRESS OF THE FIRST STORED CHANNEL: column out_cmin (a multiple of 4) of an NHWC view
 *    whose pixels are out_ld floats apart.  Only channels out_cmin .. Cout are stored, columns below are never touched; the launcher
 *    forms the view's base out - out_cmin itself, so a caller never holds a pointer outside its buffer -- neither for a full-width view
 *    (out = view + out_cmin, out_ld >= round_up(Cout, 4)) nor for a compact buffer of just the stored channels (out = the buffer,
 *    out_ld >= round_up(Cout, 4) - out_cmin).
 *  - First plane sink out_hi / out_lo (may be NULL; `out` and the sink not both NULL): the result once more as split planes at channel
 *    offset out_c0 (a multiple of 8) of a plane buffer with plane_rows >= N*H*W rows per chunk, through a per-channel PReLU of its own
 *    (plane_prelu, padded to a multiple of 32 floats, or NULL; as atmvfi_conv3x3_f16x3); plane channels from Cout up to the next
 *    multiple of 8 are written as zero.
 *  - Second, RAW plane sink out_hi2 / out_lo2 (plane_rows2 rows per chunk, channel offset out_c02, a multiple of 8; needs the first
 *    sink): a decoder map of the reference goes on twice -- through the next stage's leading nn.PReLU into that stage's deconv
 *    (network_base.py:209,215: the first sink with plane_prelu) and as it is into the refiner's strided convs (network_base.py:421-424,
 *    torch.cat([feat, dec], 1): atmvfi_gemm CONV mode with in_hi2 / in_lo2 reads it).
 *  - wn: 0 = pick the tile width (n-tiles of 16 output channels per workgroup) from the cost model, 1..8 = force it (tests, sweeps).
 *  - SPLIT-K for launches whose tiles leave most of the chip idle (small frames: the motion-MLP layers of network_lite at 256 x 256
 *    are 22 workgroups walking 200 k-steps each): with a `workspace` of at least atmvfi_conv3x3_planes_workspace_floats() floats
 *    (16-byte aligned; NULL / too small: no split) the K range is cut into up to 8 ranges of whole 32-channel chunks, one workgroup per
 *    (tile, range) writes raw fp32 partial sums into the workspace and a second kernel adds them IN RANGE ORDER and runs the epilogue
 *    (bias, PReLU, fp32 rows, plane sinks).  Run-to-run deterministic; differs from the unsplit launch by fp32 summation order only
 *    (the reference's conv, network_base.py:20-25, fixes no order either).  atmvfi_conv3x3_planes_workspace_floats returns 0 when the
 *    launcher would not split that shape on this device.
 *  - Fused READ-OUT (readout_w non-null; a mode of the same call): the tail of the refiner in two launches instead of three, without the
 *    64-channel full-resolution map r1 ever reaching HBM (network_base.py:257-260 refine_head = conv(2c, c) + PReLU, conv(c, 3) +
 *    PReLU; :429 2 * sigmoid - 1; :532-533 +=, clamp).  This call is refine_head.0 (Cout = 32 or 64: one column block) whose epilogue
 *    multiplies the activated tile -- still in registers, in the accumulator layout, which is the B-operand layout of the next MFMA --
 *    by the 27 x Cout matrix W2[(tap, o)][c] = refine_head.1's weight [o][c][tap] (f16x3 like every contraction) and stores the 27
 *    per-pixel "tap contributions" as planar fp32 readout[(tap * 3 + o) * readout_plane + pixel], readout_plane >= N*H*W.  readout_w:
 *    fp16 [plane hi / lo'][row tile 2][k-step Cout / 32][lane 64][8] in the kernel's register order, 16-byte aligned
 *    (hip_ops.HipOps.pack_readout builds it).  The tile IS the result: out, both sinks, workspace and wn must be unset (anything else:
 *    ATMVFI_EINVAL before any launch; the launcher takes wn = Cout / 16).  atmvfi_refine_tail then forms out[o][p] = bias[o] + sum over
 *    the nine taps of readout[tap * 3 + o][p + offset(tap)] (taps outside the image contribute nothing: the convolution's zero
 *    padding), PReLU(slope), 2 * sigmoid - 1, + it, and the clamped frame -- the outputs of atmvfi_final_residual.
 *  - terms, the NUMBER OF TERMS of a product: 3 = hi*hi + hi*lo' + lo'*hi (f16x3), 1 = hi*hi alone (the single-pass fp16 mode, see
 *    ATMVFI_PREC_F16: one MFMA per product into the one accumulator, same k order, same tile width and K split as with 3).  The input
 *    planes, the weight planes and every output rule are unchanged: both lo' planes must still be passed, and the plane sinks still
 *    write both planes of the launch's own fp32 result.  The read-out's 27-row W2 product on the activated tile is three-term in both:
 *    it forms the output residual and costs next to nothing.  Any other value, 0 included: ATMVFI_EINVAL before any launch. */
typedef struct atmvfi_conv3p_params {
    const void* in_hi;
    const void* in_lo;
    int64_t in_rows;
    int32_t N, H, W, Cin;
    const void* w_hi;             /* atmvfi_pack_weight_conv3x3 */
    const void* w_lo;
    int32_t Cout;
    const float* bias;            /* [Cout] or NULL */
    const float* prelu;           /* [Cout] or NULL */
    float* out;
    int32_t out_ld, out_cmin;
    void* out_hi;
    void* out_lo;
    int64_t plane_rows;
    int32_t out_c0;
    const float* plane_prelu;
    void* out_hi2;
    void* out_lo2;
    int64_t plane_rows2;
    int32_t out_c02;
    int32_t wn;
    float* workspace;
    int64_t workspace_floats;
    const void* readout_w;
    float* readout;
    int64_t readout_plane;
    int32_t terms;
} atmvfi_conv3p_params;
int atmvfi_conv3p(const atmvfi_conv3p_params* p, void* stream);
int64_t atmvfi_conv3x3_planes_workspace_floats(int N, int H, int W, int Cin, int Cout);
/* ------------------------------------------------------------------------------------
 * LayerNorm over the channel axis of token rows (eps 1e-5, affine), optional gather.
 * Replaces nn.LayerNorm at attention.py:316 (norm1 on windowed tokens), :333 (norm2) and
 * network_base.py:84 (fusion norm).  With `src_row_map` (length `rows`), output row r reads
 * source row src_row_map[r]; a negative entry denotes a zero-padded token, whose
 * LayerNorm is exactly `beta` (attention.py:58-61 pads with zeros BEFORE norm1).
 * The map fuses pad_if_needed + torch.roll + window_partition (attention.py:273-313).
 * Output sinks (also of atmvfi_dwconv3x3_gelu and atmvfi_window_attention): fp32 rows `out`, and/or the split-plane
 * pair `out_hi`/`out_lo` (fp16, chunk major with `plane_rows` rows per 32-channel chunk) that feeds atmvfi_gemm's in_hi/in_lo
 * directly -- the consumer GEMM then skips its fp32 -> fp16-pair conversion.  Either side may be NULL, not both.
 * ---------------------------------------------------------------------------------- */
int atmvfi_layernorm(const float* in, int in_ld, int64_t in_gstride, int in_rpg,
                     const int32_t* src_row_map, float* out, int out_ld,
                     const float* gamma, const float* beta, int64_t rows, int C,
                     void* out_hi, void* out_lo, int plane_rows, void* stream);

/* Depth-wise 3x3 conv (pad 1, bias) + exact GELU on NHWC tokens: DWConv + act of
 * attention.py:74-85,118-119.  weight9 is [9][C] (tap-major), see atmvfi_pack_dw_weight. */
int atmvfi_dwconv3x3_gelu(const float* in, int in_ld, float* out, int out_ld,
                          const float* weight9, const float* bias,
                          int N, int H, int W, int C, void* out_hi, void* out_lo, int plane_rows, void* stream);
int atmvfi_pack_dw_weight(const float* src /*[C,1,3,3]*/, float* dst /*[9][C]*/, int C, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused window attention (attention.py:187-213 AttentionToMotion.forward, :370-390
 * WindowAttention.forward).  qkv: [Bw*N, 3C] rows in window order, columns [q | k | v],
 * head h at columns h*hd.  One workgroup per (window, head): K/V tiles staged in LDS,
 * S^T = K Q^T and O^T = V^T P^T on fp32 MFMA, softmax by wavefront reductions; the
 * N x N attention matrix never reaches HBM.
 *   labels : optional [nW, N] int32 per-token region label; additive mask is
 *            -100 * (label_q != label_k)  (attention.py:54-57, 296-303); window index of
 *            block b is b % nW.
 *   kv_shift: K/V are read from window (b + kv_shift) % Bw -- Bw/2 for the cross-frame
 *            attention of ATMFormer (attention.py:318), 0 for self attention.
 *   motion : optional [Bw, N, heads, 2]: per-head expected key offset
 *            sum_k A[q,k] * (k_xy - q_xy)   (attention.py:207-208)
 * ---------------------------------------------------------------------------------- */
int atmvfi_window_attention(const float* qkv, float* out /*[Bw*N, C]*/, float* motion,
                            const int32_t* labels, int Bw, int nW, int ws, int heads, int hd,
                            int kv_shift, void* out_hi, void* out_lo, int plane_rows, void* stream);
/* The same contract on the f16x3 arithmetic of the contraction engines (x = hi + lo'/1024 in fp16, three
 * v_mfma_f32_16x16x32_f16 per product, fp32 accumulation: ~22 significand bits; operands beyond +-65504 saturate like
 * every other f16x3 kernel): K / V converted while they are staged, V read back through gfx950's transposing LDS read.
 * What Network.forward calls under precision "f16x3"; atmvfi_window_attention stays the exact-fp32 kernel. */
int atmvfi_window_attention_f16x3(const float* qkv, float* out /*[Bw*N, C]*/, float* motion,
                                  const int32_t* labels, int Bw, int nW, int ws, int heads, int hd,
                                  int kv_shift, void* out_hi, void* out_lo, int plane_rows, void* stream);
/* Named entry points of SURVEY.md section 8b (shims over atmvfi_window_attention). */
int atmvfi_window_attn_cross_motion(const float* qkv, float* out, float* motion, const int32_t* labels,
                                    int Bw, int nW, int ws, int heads, int hd, void* stream);
int atmvfi_window_attn_self(const float* qkv, float* out, const int32_t* labels,
                            int Bw, int nW, int ws, int heads, int hd, void* stream);

/* Head read-out of the motion (attention.py:143-146, 209-211): Linear(heads->heads/2), GELU,
 * Linear(heads/2->1) over the head axis, separately for dx and dy, then scatter from window
 * order to image order (window_reverse + roll back + de-pad, attention.py:324-331) and into
 * the channel-stacked motion map of the motion MLP input (network_base.py:377-382):
 * destination = out + (r / out_rpg) * out_gstride + (r % out_rpg) * out_ld + {0,1}, r = row_map[m]. */
int atmvfi_motion_head(const float* motion /*[rows, heads, 2]*/, const int32_t* row_map,
                       const float* w0 /*[heads/2, heads]*/, const float* b0, const float* w1 /*[1, heads/2]*/,
                       const float* b1, float* out, int out_ld, int64_t out_gstride, int out_rpg,
                       int64_t rows, int heads, void* stream);
/* The same, and the two values again as split planes (hi / lo', chunk major, plane_rows rows per chunk): row r = row_map[m] goes to plane
 * row r % out_rpg, channels plane_c0 + (r / out_rpg) * plane_gc + {0, 1} -- the eight motion channels of the motion MLP's plane input
 * (network_base.py:377-382, 410) without a separate split pass.  Channel offsets must be even. */
int atmvfi_motion_head_planes(const float* motion, const int32_t* row_map, const float* w0, const float* b0, const float* w1,
                              const float* b1, float* out, int out_ld, int64_t out_gstride, int out_rpg, int64_t rows, int heads,
                              void* out_hi, void* out_lo, int64_t plane_rows, int plane_c0, int plane_gc, void* stream);

/* ------------------------------------------------------------------------------------
 * Backward bilinear warp, zero padding (flow_warp.py:50-60 -> grid_sample(bilinear, zeros,
 * align_corners=True)); coordinates are generated in-kernel (the reference builds the
 * grid on the CPU on every call, flow_warp.py:57).
 * Flow is addressed as fx = flow[b*flow_bstride + pix*flow_pstride], fy = fx[flow_cstride],
 * which covers planar [B,2,H,W] (pstride 1, cstride H*W) and the last-5-channel NHWC
 * motion maps (pstride ld, cstride 1).
 * ---------------------------------------------------------------------------------- */
int atmvfi_flow_warp(const float* src /*[B,C,H,W]*/, const float* flow, int64_t flow_bstride,
                     int flow_pstride, int flow_cstride, float* dst, int B, int C, int H, int W, void* stream);
/* atmvfi_flow_warp with LDS-STAGED SOURCE TILES (the same signature and bit-identical results): a workgroup owns 32 x 8 output pixels,
 * stages the bounding box of their bilinear taps (up to 64 x 24 source pixels per plane, 16-byte row loads) in LDS and takes the taps
 * from there; tiles whose flows reach further gather from global memory.  Needs W % 4 == 0 and a 16-byte aligned src (ATMVFI_EINVAL
 * otherwise: the caller uses atmvfi_flow_warp). */
int atmvfi_flow_warp_tiled(const float* src /*[B,C,H,W]*/, const float* flow, int64_t flow_bstride,
                           int flow_pstride, int flow_cstride, float* dst, int B, int C, int H, int W, void* stream);
/* The reference's non-default forms of flow_warp (flow_warp.py:50-60 with mask=True and / or padding_mode != 'zeros';
 * bilinear_sample :26-47): planar flow [B,2,H,W]; padding_mode 0 'zeros', 1 'border', 2 'reflection' (grid_sample's coordinate maps,
 * align_corners=True); mask (may be NULL): [B,H,W] bytes, 1 where the normalised sampling coordinate lies in [-1, 1] on both axes
 * (flow_warp.py:43, on the reference's own fp32 expression).  Not on the forward's path. */
int atmvfi_flow_warp_ex(const float* src /*[B,C,H,W]*/, const float* flow /*[B,2,H,W]*/, float* dst, uint8_t* mask /*[B,H,W] or NULL*/,
                        int B, int C, int H, int W, int padding_mode, void* stream);
int atmvfi_flow_warp_nhwc(const float* src, int src_ld, int64_t src_bstride,
                          const float* flow, int64_t flow_bstride, int flow_pstride, int flow_cstride,
                          float* dst, int dst_ld, int64_t dst_bstride, int B, int C, int H, int W, void* stream);

/* Fused per-level synthesis (network_base.py:464-466, 496-498, 523-525): warp both frames with
 * their flows, mask = sigmoid(logit), I_t = mask*I0w + (1-mask)*I1w.  `motion` is a 5-channel
 * map [flow0.xy, flow1.xy, mask logit] with pixel stride `motion_ld` (NHWC slice).  Optional
 * outputs (NULL to skip): planar flows/masks for the returned dict, and a 15-channel NHWC
 * pack [im0, I0w, im1, I1w, I_t] into the refiner input (network_base.py:418; im0/im1 there
 * are the ORIGINAL frames `orig0/orig1`). */
int atmvfi_warp_blend(const float* im0, const float* im1 /*[B,3,H,W] (pre-warped pyramids)*/,
                      const float* motion, int motion_ld, int64_t motion_bstride,
                      float* i0w, float* i1w, float* it /*[B,3,H,W]*/,
                      float* flow0_out, float* flow1_out /*[B,2,H,W]*/, float* mask1_out, float* mask2_out /*[B,1,H,W]*/,
                      const float* orig0, const float* orig1, float* pack15, int pack_ld,
                      int B, int H, int W, void* stream);
/* The same with a plane sink for the pack: the 15 values and one zero as split planes (atmvfi_split_planes layout, pack_rows rows per
 * chunk, row = pixel b*H*W + y*W + x) at channels pack_c0 .. pack_c0 + 16 (pack_c0 a multiple of 4) -- the operand format of
 * atmvfi_conv3p, which the refiner's first conv runs on.  pack_hi / pack_lo may be NULL (= atmvfi_warp_blend). */
int atmvfi_warp_blend_planes(const float* im0, const float* im1, const float* motion, int motion_ld, int64_t motion_bstride,
                             float* i0w, float* i1w, float* it, float* flow0_out, float* flow1_out, float* mask1_out, float* mask2_out,
                             const float* orig0, const float* orig1, float* pack15, int pack_ld, void* pack_hi, void* pack_lo,
                             int64_t pack_rows, int pack_c0, int B, int H, int W, void* stream);
/* atmvfi_warp_blend_planes with LDS-staged source tiles of both images (see atmvfi_flow_warp_tiled): the same signature, bit-identical
 * results; W % 4 == 0, im0 / im1 16-byte aligned. */
int atmvfi_warp_blend_tiled(const float* im0, const float* im1, const float* motion, int motion_ld, int64_t motion_bstride,
                            float* i0w, float* i1w, float* it, float* flow0_out, float* flow1_out, float* mask1_out, float* mask2_out,
                            const float* orig0, const float* orig1, float* pack15, int pack_ld, void* pack_hi, void* pack_lo,
                            int64_t pack_rows, int pack_c0, int B, int H, int W, void* stream);
#define atmvfi_blend atmvfi_warp_blend   /* SURVEY.md section 8b name */

/* Half-resolution motion (warp.hip; ABI 0.26; the definition and the host twins: atm-vfi_amd/scaled.py).  Nothing of the reference: motion
 * is estimated on 2x reduced frames and the frame is synthesised at full size.
 * atmvfi_frame_half.  `planes` contiguous H x W fp32 planes -> H/2 x W/2: out = ((a + b) + (c + d)) * 0.25f, a b the top-row pair and c d
 *   the bottom-row pair of the 2 x 2 block (F.avg_pool2d(., 2) up to its summation order; commutes with atmvfi_frame_rot180 bit for bit).
 *   16-byte loads and stores when both pointers are 16-byte aligned and W % 8 == 0 (a lane owns four outputs), scalar accesses otherwise;
 *   the same bits.  ATMVFI_EINVAL before any launch: null pointers, planes < 1, H or W below 2 or odd, src and dst overlapping.
 * atmvfi_synth_up2.  The inputs are the half-size outputs of one forward on the reduced frames, contiguous fp32: it_sum (blend +
 *   residual, unclamped), it0, it1 (the two warped frames) [B,3,h,w]; flow0, flow1 [B,2,h,w]; m1 [B,1,h,w].  Per half-size pixel
 *       r = it_sum - (m1 * it0 + (1.0f - m1) * it1)                                  (atmvfi_warp_blend's expression)
 *   and the eight maps f0x f0y f1x f1y m1 rR rG rB are up-sampled x2 with half-pixel centres (F.interpolate(scale_factor=2, bilinear,
 *   align_corners=False)): output column x reads half columns max(x/2 - 1, 0), x/2 with weights 0.25, 0.75 when x is even and (x-1)/2,
 *   min((x+1)/2, w-1) with weights 0.75, 0.25 when x is odd, rows likewise:  v = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11),
 *   every product and sum rounded to fp32.  The flows are then doubled (exact) and, with H = 2h, W = 2w,
 *       I_t = clamp((m * warp(L, f0) + (1.0f - m) * warp(R, f1)) + r, 0, 1)
 *   where warp is atmvfi_flow_warp's (zeros padding, the reference's coordinate round trip; a non-finite flow samples 0.0 exactly),
 *   L = store0[slots0[b]] and R = store1[slots1[b]] are [3,H,W] frames of the two full-size stores [S0,3,H,W] / [S1,3,H,W] (the
 *   stores may be one; slots0 / slots1 are HOST arrays of B entries, NULL = b).  Outputs, either or both: dst_f32 [B,3,H,W], and
 *   dst_u8 [B,hh,ww,3] = the window (pad_top, pad_left, hh, ww) of the canvas as atmvfi_frame_f32_to_u8 gives it (x * 255 in fp32,
 *   round half to even, clamp; BGR if `bgr`) from the same fp32 value.  Optional f0_out, f1_out [B,2,H,W] (both or neither) and m_out
 *   [B,1,H,W]: the up-sampled, doubled flows and the up-sampled mask.
 *   One launch; a workgroup owns a 32 x 8 tile of outputs, builds the 18 x 6 half-size neighbourhood of the eight maps in LDS, and takes
 *   the sources from LDS-staged boxes as atmvfi_warp_blend_tiled does (path 2; W % 4 == 0 and 16-byte aligned stores; a tile whose flows
 *   leave the box gathers, per source) or by gathers throughout (path 1; any size).  path 0 is path 1, the faster by measurement; 2 runs
 *   on request.  The two give the same bits.  No atomics in global memory, nothing pre-zeroed, no host synchronisation; every output element is written by one lane.
 *   `workspace` is not used: atmvfi_synth_up2_workspace_floats returns 0 (or -1 for a shape the call refuses) and the pointer may be
 *   NULL.  A half-size pre-pass into an interleaved workspace was built and measured slower (README, "Half-resolution motion"); the two
 *   names stay in the ABI for a form that needs scratch.  Not for launch plans: the parameter block and the slot lists are host memory
 *   read at the call.
 *   ATMVFI_EINVAL before any launch: a null input; B < 1 or B > 16; h or w < 1; S0 or S1 < 1 or a slot outside its store; no output;
 *   one of f0_out / f1_out alone; a dst_u8 window outside the canvas; an unknown path, or path 2 where it is not allowed; an output that
 *   overlaps an input or another output. */
int atmvfi_frame_half(const float* src, float* dst, int planes, int H, int W, void* stream);
typedef struct atmvfi_synth_up2_params {
    const float *it_sum, *it0, *it1;     /* [B,3,h,w] */
    const float *flow0, *flow1;          /* [B,2,h,w] */
    const float* m1;                     /* [B,1,h,w] */
    const float *store0, *store1;        /* [S0,3,2h,2w], [S1,3,2h,2w] */
    const int32_t *slots0, *slots1;      /* host arrays of B entries, or NULL */
    float* dst_f32;                      /* [B,3,2h,2w] or NULL */
    void* dst_u8;                        /* [B,hh,ww,3] or NULL */
    float *f0_out, *f1_out, *m_out;      /* optional */
    float* workspace;                    /* unused, may be NULL */
    int32_t B, h, w, S0, S1;
    int32_t pad_top, pad_left, hh, ww, bgr;   /* read only with dst_u8 */
    int32_t path;                        /* 0 auto (= 1), 1 gathers, 2 staged boxes */
    int32_t reserved;
} atmvfi_synth_up2_params;
int atmvfi_synth_up2(const atmvfi_synth_up2_params* p, void* stream);
int64_t atmvfi_synth_up2_workspace_floats(int B, int h, int w);

/* Bilinear resize with align_corners=True, src = dst*(in-1)/(out-1), values * value_scale:
 * F.interpolate(scale 0.5) of the image pyramid (network_base.py:445-446,461-462) and
 * upsample_flow (network_base.py:11-18, value_scale = factor).  Source element (b,c,y,x) is
 * src[b*sb + c*sc + y*sy + x*sx] (planar NCHW or a channel slice of an NHWC motion map);
 * dst is planar contiguous [B,C,Ho,Wo]. */
int atmvfi_resize_bilinear_ac(const float* src, int64_t src_bstride, int64_t src_cstride, int64_t src_ystride,
                              int64_t src_xstride, float* dst, int B, int C, int Hi, int Wi, int Ho, int Wo,
                              float value_scale, void* stream);

/* The three x0.5 levels of the image pyramid of both frames (network_base.py:444-448) in one launch: im0 / im1 planar [B,3,H,W]
 * (H, W >= 8); l1 / l2 / l3 planar [2B,3,H>>l,W>>l], frame 0's images first.  Bit-identical to atmvfi_resize_bilinear_ac
 * applied level by level. */
int atmvfi_image_pyramid(const float* im0, const float* im1, float* l1, float* l2, float* l3, int B, int H, int W, void* stream);
/* The same and, with `pack` non-NULL, atmvfi_pack_frames' output [2B,H,W,4] in the same launch (both read only the two frames). */
int atmvfi_image_pyramid_pack(const float* im0, const float* im1, float* l1, float* l2, float* l3, float* pack, int B, int H, int W,
                              void* stream);

/* flow_warp (flow_warp.py:50-60) of a planar image [B,C,H,W] by a contiguous planar flow [B,2,H,W] into dst, AND that flow up-sampled
 * to [B,2,2H,2W] with its values doubled (upsample_flow, network_base.py:11-18) into flow_up, in one launch: one step of the global
 * flow's walk down the image pyramid (network_base.py:468-485).  Bit-identical to atmvfi_flow_warp + atmvfi_resize_bilinear_ac(x2). */
int atmvfi_flow_warp_up2(const float* src, const float* flow, float* dst, float* flow_up, int B, int C, int H, int W, void* stream);
/* The same with the warp half on LDS-staged source tiles (atmvfi_flow_warp_tiled): bit-identical; W % 4 == 0, src 16-byte aligned. */
int atmvfi_flow_warp_up2_tiled(const float* src, const float* flow, float* dst, float* flow_up, int B, int C, int H, int W, void* stream);

/* torch.cat([im0, im1], 0) (network_base.py:451) fused with NCHW -> NHWC4 (4th channel 0). */
int atmvfi_pack_frames(const float* im0, const float* im1, float* dst /*[2B,H,W,4]*/, int B, int H, int W, void* stream);

/* I_t += 2*sigmoid(r) - 1; clamp(0,1) (network_base.py:429,532-533).  `r` is the NHWC 3-channel
 * output of refine_head; writes the unclamped sum (the tensor the reference leaves in
 * im_t_list[0]) and the clamped frame. */
int atmvfi_final_residual(const float* it /*[B,3,H,W]*/, const float* r, int r_ld,
                          float* it_sum, float* it_clamped, int B, int H, int W, void* stream);

/* The second launch of the refiner's tail: the gather over the read-out of atmvfi_conv3p (atmvfi_conv3p_params, "Fused READ-OUT");
 * contrib / contrib_plane are that call's readout / readout_plane. */
int atmvfi_refine_tail(const float* contrib, int64_t contrib_plane, const float* bias /*[3] or NULL*/, const float* slope /*[3] or NULL*/,
                       const float* it /*[B,3,H,W]*/, float* it_sum, float* it_clamped, int B, int H, int W, void* stream);

/* Host-boundary frame formats (demo_2x.py:64-85 inference_2frame + benchmark/utils.py:57-80 InputPadder), SURVEY 8f-2.
 *   u8_to_f32: uint8 [H,W,3] (BGR if `bgr`, as cv2 delivers) -> fp32 planar RGB [3,Hp,Wp] = x / 255 with replicate padding,
 *              the source frame sitting at (pad_top, pad_left) of the padded canvas;
 *   f32_to_u8: the inverse: crop, np.round(x * 255) (half to even), uint8 [H,W,3].  Bit-exact against the numpy path. */
int atmvfi_frame_u8_to_f32(const void* src, int H, int W, int bgr, float* dst, int Hp, int Wp, int pad_top, int pad_left, void* stream);
int atmvfi_frame_f32_to_u8(const float* src, int Hp, int Wp, int pad_top, int pad_left, void* dst, int H, int W, int bgr, void* stream);
/* One resident uint8 [H,W,3] frame (contiguous; BGR if `bgr`) -> the h x w output window that a dataset evaluation needs, as a network
 * input and / or a ground truth (benchmark/test_xiph.py of the reference: "cropped-4k" and "resized-2k").
 *   mode 0 (crop):    output pixel (y, x) = src[y0 + y, x0 + x];
 *   mode 1 (area 2x): output pixel (y, x) = (a + b + c + d + 2) >> 2 per channel over the 2x2 source block at (y0 + 2y, x0 + 2x) --
 *                     cv2.INTER_AREA for uint8 at an exact scale of 2, ties round up; the window covers 2h x 2w source pixels.
 *   dst    (or NULL): fp32 planar RGB [3,Hp,Wp] = q / 255 (a true fp32 division) with replicate padding, the window at (pad_top, pad_left);
 *   dst_u8 (or NULL): uint8 [h,w,3] RGB, the same integer pixels, un-padded: the ground truth form atmvfi_ssim_psnr reads in place.
 * Not both NULL.  Any geometry and pointer alignment is accepted; dword loads and 16-byte plane stores are used when src and dst_u8 are
 * 4-byte and dst 16-byte aligned and W, x0, w, pad_left and Wp are multiples of 4.  Both paths give the same bits. */
int atmvfi_frame_u8_window(const void* src, int H, int W, int bgr, int mode, int y0, int x0, int h, int w, float* dst, int Hp, int Wp,
                           int pad_top, int pad_left, void* dst_u8, void* stream);

/* Multi-frame (4x / 8x recursive) interpolation, benchmark/davis-vid.py:98-135 of the reference: a pool of per-frame state and the
 * flip-TTA tail.
 * atmvfi_pool_blocks: n (1..32) blocks of block_bytes between pool slots and one contiguous buffer, in one launch.
 *   gather  (to_pool 0): buf block j = the first block_bytes of pool + slots[j] * slot_bytes; a slot may be named more than once;
 *   scatter (to_pool 1): the inverse; a slot named twice is rejected.
 *   `slots` is a HOST array of n entries, read during the call (it travels in the kernel arguments: no device table, no copy, and the
 *   launch can be captured).  pool and buf 16-byte aligned, slot_bytes and block_bytes multiples of 16, block_bytes <= slot_bytes,
 *   0 <= slots[j] < n_slots; the pool spans n_slots * slot_bytes, buf n * block_bytes.  Everything is checked on the host.
 * atmvfi_tta_merge: out = (pred + rot180(pred_flip)) / 2 in fp32 -- the bits of (pred + pred_flip.flip(H).flip(W)) / 2 -- and / or
 *   out_u8 = atmvfi_frame_f32_to_u8 of it (crop at (pad_top, pad_left), x * 255 in fp32, round half to even, clamp, RGB -> BGR if
 *   `bgr`).  Not both NULL; H, W, pad_* are read only with out_u8.  Any alignment; 16-byte accesses when Hp * Wp % 4 == 0 and the fp32
 *   pointers are 16-byte aligned.  Same bits either way.
 * atmvfi_frame_rot180: dst = src.flip(H).flip(W) of C contiguous planes (the flattened reversal of each plane); not in place. */
int atmvfi_pool_blocks(void* pool, int64_t slot_bytes, int n_slots, const int32_t* slots /*HOST array, n entries*/, int n /*1..32*/,
                       int64_t block_bytes, void* buf, int to_pool, void* stream);
int atmvfi_tta_merge(const float* pred /*[3,Hp,Wp]*/, const float* pred_flip /*[3,Hp,Wp]*/, float* out /*[3,Hp,Wp] or NULL*/,
                     void* out_u8 /*uint8 [H,W,3] or NULL*/, int Hp, int Wp, int pad_top, int pad_left, int H, int W, int bgr, void* stream);
int atmvfi_frame_rot180(const float* src /*[C,Hp,Wp]*/, float* dst, int C, int Hp, int Wp, void* stream);

/* Frame signature for scene-cut detection in the video loops (scene.hip; atm-vfi_amd/scene.py compares two of them).  Nothing of the
 * reference: its scripts only see single-shot clips.  One resident uint8 [H,W,3] frame (contiguous; BGR if `bgr`) and the window
 * (y0, x0, h, w) -> int32 sig[288] on the device:
 *   luma          Y = (77 R + 150 G + 29 B + 128) >> 8;
 *   sig[16 i + j] = the sum of Y over rows [i h / 16, (i + 1) h / 16) and columns [j w / 16, (j + 1) w / 16) of the window (integer
 *                   division: a 16 x 16 grid of cells, row-major);
 *   sig[256 + b]  = the number of window pixels with Y >> 3 == b (32 bins).
 * h, w >= 16, the window inside the frame, and small enough that cell sums and bin counts fit int32 (ATMVFI_EINVAL otherwise).  Any
 * geometry and pointer alignment of src is accepted; dword loads are used when src is 4-byte aligned and W, x0 and w are multiples of 4.
 * Integer arithmetic only: both paths and any reduction order give the same bits.  sig (4-byte aligned) is written completely by the
 * call: nothing is pre-zeroed and no global atomics are used.  workspace: at least atmvfi_frame_signature_workspace_ints(h, w) int32 of
 * scratch, the caller's (per-workgroup partials, reduced by a second launch of the same call); the query returns -1 for a window the
 * call would refuse.  Stream-ordered: two launches, no host synchronisation, no allocation. */
int64_t atmvfi_frame_signature_workspace_ints(int h, int w);
int atmvfi_frame_signature(const void* src, int H, int W, int bgr, int y0, int x0, int h, int w, int32_t* sig /*[288]*/, int32_t* workspace,
                           int64_t workspace_ints, void* stream);

/* Frame difference for duplicate-frame detection in the retimed video loop (framediff.hip; ABI 0.16; atm-vfi_amd/retime.py judges it).
 * Nothing of the reference.  Two resident uint8 [H,W,3] frames a and b of the same geometry (contiguous; BGR if `bgr`) and the window
 * (y0, x0, h, w) -> int32 out[258] on the device:
 *   luma          Y = (77 R + 150 G + 29 B + 128) >> 8 (the signature's);
 *   out[16 i + j] = the sum of |Ya - Yb| over rows [i h / 16, (i + 1) h / 16) and columns [j w / 16, (j + 1) w / 16) of the window (the
 *                   signature's 16 x 16 cells, row-major);
 *   out[256]      = the maximum of |Ya - Yb| over the window;
 *   out[257]      = the number of window pixels with Ya != Yb.
 * The window rules and refusals of atmvfi_frame_signature: h, w >= 16, the window inside the frame, and small enough that cell sums and
 * the pixel count fit int32 (ATMVFI_EINVAL otherwise).  Any geometry and pointer alignment of a and b is accepted; dword loads are used
 * when BOTH are 4-byte aligned and W, x0 and w are multiples of 4.  Integer arithmetic only: both paths and any reduction order give the
 * same bits.  out (4-byte aligned) is written completely by the call: nothing is pre-zeroed and no global atomics are used.  workspace:
 * at least atmvfi_frame_difference_workspace_ints(h, w) int32 of scratch, the caller's (per-workgroup partials, reduced by a second
 * launch of the same call); the query returns -1 for a window the call would refuse.  Stream-ordered: two launches, no host
 * synchronisation, no allocation. */
int64_t atmvfi_frame_difference_workspace_ints(int h, int w);
int atmvfi_frame_difference(const void* a, const void* b, int H, int W, int bgr, int y0, int x0, int h, int w, int32_t* out /*[258]*/,
                            int32_t* workspace, int64_t workspace_ints, void* stream);

/* Active picture of letterboxed video in the N-x loop (active.hip; ABI 0.21; atm-vfi_amd/active.py holds the policy and the host twins
 * borders_numpy / compose_numpy; per-pixel model tests/cpu_active.py).  Nothing of the reference.
 * atmvfi_frame_borders: one resident uint8 [H,W,3] frame (contiguous; BGR if `bgr`) -> int32 out[H + W] on the device:
 *   luma       Y = (77 R + 150 G + 29 B + 128) >> 8 (the signature's);
 *   out[y]     = the maximum of Y over row y;      out[H + x] = the maximum of Y over column x.
 *   H, W >= 16, H * W fits int32 and the frame has at most 65535 row chunks (ATMVFI_EINVAL otherwise).  Any pointer alignment of src is
 *   accepted; dword loads are used when src is 4-byte aligned and W is a multiple of 4.  Integer arithmetic only: both paths and any
 *   reduction order give the same bits.  out (4-byte aligned) is written completely by the call: nothing is pre-zeroed and no global
 *   atomics are used.  workspace: at least atmvfi_frame_borders_workspace_ints(H, W) int32 of scratch, the caller's (per-wave row
 *   maxima and per-chunk column maxima, reduced by a second launch of the same call); the query returns -1 for a frame the call would
 *   refuse.  Stream-ordered: two launches, no host synchronisation, no allocation.
 * atmvfi_frame_compose: dst uint8 [H,W,3] = a produced window put back into a full frame.  Outside the window (y0, x0, h, w) -- h, w >=
 *   1, inside the frame -- the bytes of `border`, a resident uint8 [H,W,3] frame in the caller's channel order, verbatim.  Inside, from
 *   exactly one of: src, fp32 planar RGB [3,Hp,Wp] with the window at (pad_top, pad_left) -- atmvfi_frame_f32_to_u8's pixel (x * 255 in
 *   fp32, round half to even, clamp, RGB -> BGR if `bgr`); win_u8, uint8 [h,w,3] already in output order (what atmvfi_tta_merge
 *   writes; `bgr`, Hp, Wp, pad_* are not read).  dst must not overlap border (ATMVFI_EINVAL).  Only the bar region of border and the
 *   window of src / win_u8 are read.  Any geometry and alignment; 12-byte RGB groups and 16-byte plane reads when dst, border and
 *   win_u8 are 4-byte aligned, W, x0 and w multiples of 4 and, with src, src 16-byte aligned and Wp, pad_left multiples of 4.  Same bits
 *   either way.  One launch. */
int64_t atmvfi_frame_borders_workspace_ints(int H, int W);
int atmvfi_frame_borders(const void* src, int H, int W, int bgr, int32_t* out /*[H + W]*/, int32_t* workspace, int64_t workspace_ints,
                         void* stream);
int atmvfi_frame_compose(void* dst /*uint8 [H,W,3]*/, const void* border /*uint8 [H,W,3]*/, int H, int W, int y0, int x0, int h, int w,
                         const float* src /*[3,Hp,Wp] or NULL*/, int Hp, int Wp, int pad_top, int pad_left,
                         const void* win_u8 /*uint8 [h,w,3] or NULL*/, int bgr, void* stream);

/* The active picture on YUV streams and in the retimed loop (active.hip, yuv_encode.hip; ABI 0.22; atm-vfi_amd/active.py: bar_code,
 * yuv_borders_numpy / yuv_compose_numpy; per-sample models tests/cpu_yuv_active.py).  Nothing of the reference.  The frames are those of
 * the frame descriptor below (atmvfi_yuv_desc: depth, subsampling, chroma, msb, pitch / chroma_pitch / chroma_offset in BYTES, 0: tight).
 * atmvfi_yuv_borders: the LUMA plane of one resident frame -> int32 out[H + W] on the device (of the descriptor it reads H, W, depth,
 *   msb and pitch):
 *   out[y]     = the largest luma sample VALUE of row y (the stored sample, >> 6 with msb);   out[H + x] = that of column x.
 *   The maximum commutes with every monotone map, so raw codes are reported and the host maps its threshold once (active.bar_code).
 *   depth 8 or 10, msb only at depth 10, pitch a multiple of the sample size and at least a row's bytes (0: tight); chroma layout and
 *   subsampling do not matter: only the H rows of W samples are read, never a padding byte.  H, W >= 16, H * W fits int32, at most
 *   65535 row chunks (ATMVFI_EINVAL otherwise, checked on the host before the launch).  Any pointer alignment and pitch is accepted;
 *   the vector path (a lane's four samples as one dword or one 8-byte load) runs when the pointer and the pitch are multiples of 4
 *   bytes and W is a multiple of 4.  Both paths give the same bits.  out (4-byte aligned) is written completely by the call: nothing
 *   is pre-zeroed, no global atomics, vector stores only.  workspace: at least atmvfi_yuv_borders_workspace_ints(H, W) int32 of
 *   scratch, the caller's; the query returns -1 for a frame the call would refuse.  Stream-ordered: a partial launch and a reduce
 *   launch, no host synchronisation, no allocation.
 * atmvfi_yuv_compose: dst = ONE TIGHT frame of (H, W, depth, subsampling, chroma, msb), a produced window put back into a full frame.
 *   `border_desc` describes `border`, a resident surface of that size, depth, subsampling, chroma layout and msb; its pitch /
 *   chroma_pitch / chroma_offset are the border's own (the uploaded source frame in place), dst is that frame without them.
 *   Outside the window (y0, x0, h, w) dst gets the sample values of `border`:
 *   plane by plane, the stored samples as they are (of an msb word the value's ten bits; the low six leave as zero) --
 *   yuv.repack(border, surface, surface.tight()) outside the window.  Inside, exactly the samples
 *   atmvfi_yuv_encode writes for the h x w picture as a frame of the cropped format (matrix, full_range, siting; chroma sums clamp
 *   at the WINDOW's edges), from exactly one of: src, the fp32 canvas [3,Hp,Wp] with the window at (pad_top, pad_left); src_u8, uint8
 *   [h,w,3] RGB (depth 8 only).  The encode arithmetic is that kernel itself, launched with the window's origin in the frame.
 *   Window rule: y0 and x0 are multiples of the subsampling step per axis, y0 + h and x0 + w are multiples of it or equal H / W: every
 *   chroma sample belongs wholly to the window or wholly to the bars.  dst must not overlap border (ATMVFI_EINVAL).  Only the bar
 *   region of border and the window of the source are read; every output sample is written by exactly one lane, vector stores only,
 *   no padding byte exists in dst.  Any geometry, pitch and alignment is accepted; the vector paths run under the conditions of the
 *   decoder surfaces below with x0 a multiple of 4 as well (bars: dst, border and its strides multiples of 4 bytes).  Same bits either way.
 *   At most two launches (the bars; the window -- none for a window that is the frame / bars that are empty).  All checks run on
 *   the host before the first launch (ATMVFI_EINVAL). */
int64_t atmvfi_yuv_borders_workspace_ints(int H, int W);
struct atmvfi_yuv_desc;
int atmvfi_yuv_borders(const struct atmvfi_yuv_desc* desc, const void* yuv, int32_t* out /*[H + W]*/, int32_t* workspace,
                       int64_t workspace_ints, void* stream);
int atmvfi_yuv_compose(const struct atmvfi_yuv_desc* border_desc, void* dst, const void* border, int y0, int x0, int h, int w,
                       const float* src /*[3,Hp,Wp] or NULL*/, int Hp, int Wp, int pad_top, int pad_left,
                       const void* src_u8 /*uint8 [h,w,3] or NULL*/, void* stream);

/* Synthetic shutter for the retimed video loop (shutter.hip; ABI 0.18; atm-vfi_amd/shutter.py holds the definition -- which samples an
 * output integrates -- and the host twin blend_numpy).  Nothing of the reference.  A blurred output is the weighted mean of the uint8 RGB
 * pixels q_k of its samples, taken in the domain of a light table and brought back to the nearest code, per channel:
 *   acc = sum w_k LUT[q_k];  v = (acc + (Wt >> 1)) / Wt (floor), Wt = sum w_k;  out = the number of k in 1..255 with v >= thr[k],
 *   thr[k] = (LUT[k - 1] + LUT[k] + 1) >> 1.   1 <= Wt <= 32767 keeps 65535 Wt inside int32.
 *   light 0 "code":   LUT[q] = 257 q (the plain average of code values);
 *   light 1 "linear": LUT[q] = rint(65535 eotf(q / 255)), the sRGB curve (x / 12.92 up to 0.04045, else ((x + 0.055) / 1.055)^2.4) in
 *                     float64; strictly increasing, so out(LUT[q]) == q under both tables.
 * atmvfi_shutter_accumulate: acc[c][y][x] (=, when `first`; else +=) weight * LUT[q] for one sample; acc is int32 planar [3,h,w], always
 *   R, G, B.  Exactly one source: src, fp32 planar RGB [3,Hp,Wp] with the h x w window at (pad_top, pad_left) -- q is
 *   atmvfi_frame_f32_to_u8's pixel clamp(rint(x * 255)), half to even; finite inputs, values outside [0, 1] clamp -- or src_u8, uint8
 *   [h,w,3] (B, G, R if `bgr`), q the byte.  `first` writes without reading: nothing is pre-zeroed, and a poisoned accumulator is legal
 *   input then.
 * atmvfi_shutter_resolve: the rounding division and the inverse above, acc -> dst_u8 uint8 [h,w,3] (B, G, R if `bgr`).  No data-dependent
 *   loop: one read of a 256-entry bucket table (the count for v & ~255) and four compare-and-step reads among the at most 15 thresholds
 *   that one bucket of 256 values holds.
 * atmvfi_shutter_table: the library's literal table of `light`, copied into a host buffer (no launch).
 * Refused on the host before any launch (ATMVFI_EINVAL): null pointers; both or neither source; h, w < 1; the window not inside the canvas;
 * weight < 1; total_weight outside 1..32767; an unknown light; acc (or src) not 4-byte aligned; a work-item count that does not fit an int.
 * Any geometry and pointer alignment is accepted otherwise; 16-byte plane accesses and 12-byte RGB groups are used when acc and the fp32
 * pointer are 16-byte and the byte pointers 4-byte aligned and w, Wp and pad_left are multiples of 4.  Both paths give the same bits.
 * Every output word and byte is written by exactly one lane: vector stores only, no atomics. */
int atmvfi_shutter_accumulate(int32_t* acc /*[3,h,w] planar*/, int h, int w, const float* src, int Hp, int Wp, int pad_top, int pad_left,
                              const uint8_t* src_u8 /*[h,w,3]*/, int bgr, int weight, int light, int first, void* stream);
int atmvfi_shutter_resolve(const int32_t* acc, int h, int w, int total_weight, int light, uint8_t* dst_u8 /*[h,w,3]*/, int bgr, void* stream);
int atmvfi_shutter_table(int light, uint16_t out[256]);

/* Planar YUV 4:2:0 (I420) <-> RGB for the video loops (yuv.hip decodes, yuv_encode.hip encodes, yuv_common.h holds the definition and
 * the shared helpers; atm-vfi_amd/yuv.py holds the format, the numpy twins and Y4M I/O).
 * Nothing of the reference: its scripts read PNGs.  A bit-exact contract in int32 (>> is an arithmetic shift: floor).
 * Frame: one contiguous buffer Y [H,W], U [ch,cw], V [ch,cw], ch = (H + 1) / 2, cw = (W + 1) / 2, H, W >= 1 (odd sizes allowed);
 *   uint8 samples for depth 8, little-endian uint16 with values 0..1023 for depth 10 (decode only).
 * Parameters: matrix 0 bt601 / 1 bt709; full_range 0 / 1 (10-bit full range is refused); siting 0 centre ("420jpeg") / 1 left
 *   ("420mpeg2").  Coefficients: rint(c * 2^14) of the float64 matrices of (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722), limited
 *   range scaled by 219 / 224:            decode [kY, kRV, kGU, kGV, kBU]        encode rows Y / U / V over (R, G, B)
 *     bt601 limited   19077, 26149,  -6419, -13320, 33050    (4207,  8260, 1604) / (-2428, -4768, 7196) / (7196, -6026, -1170)
 *     bt601 full      16384, 22970,  -5638, -11700, 29032    (4899,  9617, 1868) / (-2765, -5427, 8192) / (8192, -6860, -1332)
 *     bt709 limited   19077, 29372,  -3494,  -8731, 34610    (2991, 10064, 1016) / (-1649, -5547, 7196) / (7196, -6536,  -660)
 *     bt709 full      16384, 25802,  -3069,  -7670, 30402    (3483, 11718, 1183) / (-1877, -6315, 8192) / (8192, -7441,  -751)
 * Decode, chroma of luma pixel (y, x), plane c:
 *   rows (always centre-sited) r0 = y >> 1, r1 = clamp(r0 + (y & 1 ? 1 : -1), 0, ch - 1), weights (wy0, wy1) = (3, 1);
 *   columns, centre: q0 = x >> 1, q1 = clamp(q0 + (x & 1 ? 1 : -1), 0, cw - 1), weights (3, 1);
 *   columns, left:   q0 = x >> 1, q1 = min(q0 + 1, cw - 1), weights (4, 0) for even x and (2, 2) for odd x;
 *   c' = (wy0 (wx0 c[r0][q0] + wx1 c[r0][q1]) + wy1 (wx0 c[r1][q0] + wx1 c[r1][q1]) + 8) >> 4.
 * Decode, matrix: y = Y - yo, u = U' - mid, v = V' - mid; 8 bit: yo = 16 (limited) or 0 (full), mid = 128, T = 14; 10 bit: yo = 64,
 *   mid = 512, T = 16;  R = clip8((kY y + kRV v + 2^(T-1)) >> T), G = clip8((kY y + kGU u + kGV v + 2^(T-1)) >> T),
 *   B = clip8((kY y + kBU u + 2^(T-1)) >> T).
 * Encode (8 bit only): the source pixel p is the uint8 RGB value; from an fp32 source it is clamp(rint(x * 255)), half to even:
 *   atmvfi_frame_f32_to_u8's pixel.  Y = clip8(((eY . p + 2^13) >> 14) + yo).  Chroma sample (j, i) takes the un-rounded per-channel
 *   sums s over rows 2j and min(2j + 1, H - 1) and columns 2i, min(2i + 1, W - 1) with weights 1 (centre; sh = 2) or max(2i - 1, 0),
 *   2i, min(2i + 1, W - 1) with weights 1, 2, 1 (left; sh = 3):  U = clip8(((eU . s + 2^(13 + sh)) >> (14 + sh)) + 128), V with eV.
 * Decode of the whole frame (atmvfi_yuv_decode, window = the frame, mode 0): dst_u8 (or NULL) uint8 [H,W,3], BGR if `bgr`; dst (or NULL)
 *   fp32 planar RGB [3,Hp,Wp] = q / 255 (a true fp32 division) with replicate padding, the frame at (pad_top, pad_left): the bits of
 *   atmvfi_frame_u8_to_f32 applied to dst_u8.  Not both NULL; Hp, Wp and the padding are read only with dst (4-byte aligned).
 * Encode at depth 8 (atmvfi_yuv_encode): exactly one of src_u8 (uint8 [H,W,3], BGR if `bgr`) and src (fp32 planar RGB [3,Hp,Wp], the
 *   frame at (pad_top, pad_left), 4-byte aligned) -> yuv.
 * Any geometry and pointer alignment is accepted (for odd W the U plane starts at an odd byte); dword Y accesses, 16-byte plane
 * accesses and 12-byte RGB groups are used when the byte pointers are 4-byte and the fp32 pointer 16-byte aligned and W, Wp and
 * pad_left are multiples of 4.  Both paths give the same bits.  Every output byte is written by the call; no atomics, nothing
 * pre-zeroed.  All checks run on the host before the launch (ATMVFI_EINVAL).
 *
 * A window of a packed I420 frame -> the window of atmvfi_frame_u8_window, without the RGB frame in between (atmvfi_yuv_decode with
 * `mode`; yuv.hip; the Xiph 2K / 4K evaluation on Y4M clips, atm-vfi_amd/evaluate.py; host twin yuv.window_numpy).  Nothing of the
 * reference: its script converts the clips to rgb24 PNGs with ffmpeg first.  10-bit samples decode to clip8 RGB.  No new arithmetic:
 * let q(Y, X) be the clip8 RGB pixel that the whole-frame decode above gives at (Y, X) of the WHOLE H x W frame -- chroma neighbours
 * clamp at the frame's edges, never at the window's --
 *   mode 0 (crop):    out(y, x) = q(y0 + y, x0 + x);
 *   mode 1 (area 2x): out(y, x) = (q(y0 + 2y, x0 + 2x) + q(y0 + 2y, x0 + 2x + 1) + q(y0 + 2y + 1, x0 + 2x) + q(y0 + 2y + 1, x0 + 2x + 1) + 2) >> 2
 *                     per channel: the four pixels are clipped to 8 bits first and averaged then (an rgb24 picture, then cv2.INTER_AREA
 *                     at an exact scale of 2, ties round up); the window covers 2h x 2w source pixels;
 *   dst    (or NULL): fp32 planar RGB [3,Hp,Wp] = out / 255 with the bits of the fp32 division, the window at (pad_top, pad_left),
 *                     replicate padding by clamping the output coordinate into the window (4-byte aligned; Hp, Wp and the padding are
 *                     read only with dst);
 *   dst_u8 (or NULL): uint8 [h,w,3] RGB, the same integer pixels, un-padded: the ground truth form atmvfi_ssim_psnr reads in place.
 * Both are bit for bit atmvfi_frame_u8_window(mode, y0, x0, h, w, ...) of the whole-frame decode's dst_u8.
 * Refused on the host before any launch (ATMVFI_EINVAL): a null source; both outputs NULL; H or W below 1, an unknown matrix, range,
 * siting or depth; 10-bit full range; a mode other than 0 / 1; mode 1 on anything but a packed planar LSB 4:2:0 frame to pixels
 * 0..255; h, w < 1 or a negative origin; a window that leaves the frame (2h x 2w source pixels in mode 1); an odd y0 or x0 (an even
 * origin keeps the two luma rows and columns of a chroma sample together, as yuv.crop requires); a canvas smaller than the window
 * plus its padding.
 * Any geometry and pointer alignment is accepted otherwise; dword Y loads, 16-byte plane stores and 12-byte RGB groups are used when the
 * byte pointers are 4-byte and the fp32 pointer 16-byte aligned and W, x0, w, Wp and pad_left are multiples of 4.  Both paths give the
 * same bits.  Every output byte is written by the call; vector stores only, no atomics, nothing pre-zeroed.
 *
 * The same frames with the 10-bit depth kept end to end (depth 10; decode with keep_depth 1, encode from src): 10-bit limited-range
 * I420 (little-endian uint16, values 0..1023; frame layout, matrix and siting as above) <-> fp32 planar RGB in units of 1 / 1023.
 * Without keep_depth a decode takes 10-bit samples to clip8 RGB; with it the network gets q / 1023, and the encode writes its
 * prediction back as 10-bit samples.  The project's own bit-exact contract in int32 (>> floors); yuv.decode_numpy_f32 /
 * yuv.encode_numpy give the same bits on the host.
 * Coefficients: rint(c * 2^14) of the same float64 matrices, luma scaled by 876 / 1023 and chroma by 896 / 1023:
 *                       decode [kY, kRV, kGU, kGV, kBU]        encode rows Y / U / V over (R, G, B)
 *     bt601 10 bit    19133, 26226,  -6438, -13359, 33148    (4195,  8235, 1599) / (-2421, -4754, 7175) / (7175, -6008, -1167)
 *     bt709 10 bit    19133, 29459,  -3504,  -8757, 34711    (2983, 10034, 1013) / (-1644, -5531, 7175) / (7175, -6517,  -658)
 * Decode with keep_depth: chroma upsampling exactly as above (rows, columns, weights for both sitings, (.. + 8) >> 4) on the 10-bit
 *   samples; y = Y - 64, u = U' - 512, v = V' - 512; R10 = clip(0, 1023, (kY y + kRV v + 2^13) >> 14),
 *   G10 = clip(0, 1023, (kY y + kGU u + kGV v + 2^13) >> 14), B10 = clip(0, 1023, (kY y + kBU u + 2^13) >> 14); dst fp32 planar RGB
 *   [3,Hp,Wp] = q / 1023 with the bits of the fp32 division.  The call decodes the window (y0, x0, h, w) of the H x W frame -- inside the
 *   frame, even origin -- to (pad_top, pad_left) of the canvas, replicate padding by clamping the output coordinate into the window.
 *   The window is a window of the whole frame's decode: chroma neighbours clamp at the frame's edges, not the window's.
 * Encode at depth 10: src fp32 planar RGB [3,Hp,Wp], the frame at (pad_top, pad_left); source pixel p = clip(0, 1023,
 *   rint(fl32(x * 1023))), half to even (finite inputs; values outside [0, 1] clamp); Y = clip(0, 1023, ((eY . p + 2^13) >> 14) + 64);
 *   chroma from the un-rounded sums s with the taps and sh of the 8-bit encode: U = clip(0, 1023, ((eU . s + 2^(13 + sh)) >> (14 + sh))
 *   + 512), V with eV.
 * Any geometry and pointer alignment of the frame is accepted; the fp32 pointer must be 4-byte aligned.  8-byte Y accesses, dword
 * chroma pairs and 16-byte plane accesses are used when the frame pointer is 4-byte and the fp32 pointer 16-byte aligned and W, Wp,
 * pad_left (and x0, w) are multiples of 4.  Both paths give the same bits.  Every output byte and word is written by the call; no
 * atomics, nothing pre-zeroed.  All checks run on the host before the launch (ATMVFI_EINVAL).
 *
 * Decoder surfaces: NV12 / NV21 / P010 and pitched frames (atm-vfi_amd/yuv.py: Surface holds the definition on the host).  The pixel
 * arithmetic is the one above, unchanged; what differs is where the samples lie.
 * One frame is one buffer of samples (uint8, or little-endian uint16 at depth 10):
 *   chroma         0: planar, the U plane then the V plane (I420); 1: one plane of interleaved pairs, U first (NV12, P010); 2: the
 *                  same, V first (NV21)
 *   msb            depth 10 only (refused at depth 8): a stored sample is value << 6 (P010); decoding takes s >> 6 and ignores the low six
 *                  bits, encoding writes v << 6 with the low bits zero
 *   pitch, chroma_pitch   row strides in BYTES of the luma rows and of the chroma rows: multiples of the sample size, at least the row's
 *                  own bytes (W b; cw b planar, 2 cw b interleaved; b = 1 or 2).  0: tight
 *   chroma_offset  the byte offset of the first chroma row: a multiple of the sample size, at least pitch * H.  0: pitch * H.  The
 *                  planar V plane follows U at chroma_offset + chroma_pitch * ch.
 * The buffer ends with the last chroma row's own bytes; padding bytes are never read.
 * atmvfi_yuv_decode: the window (y0, x0, h, w) of the surface -- inside the frame, even origin -- to (pad_top, pad_left) of dst
 *   (fp32 planar RGB [3,Hp,Wp], replicate padding by clamping the output coordinate into the window) and / or to dst_u8 (uint8 [h,w,3],
 *   BGR if `bgr`); chroma neighbours clamp at the FRAME's edges.  keep_depth 0: clip8 RGB and q / 255 from samples of either depth;
 *   keep_depth 1 (depth 10, dst only): q / 1023.  The layout changes no sample's value: every surface of a frame decodes to the bytes of
 *   its tight planar frame.
 * atmvfi_yuv_encode: exactly one of src_u8 (uint8 [H,W,3], BGR if `bgr`; depth 8 only) and src (the fp32 canvas, the frame at
 *   (pad_top, pad_left)) -> a TIGHT surface of `chroma` / `msb` (the three strides are not read): the samples of the planar encode
 *   of its depth.  No padding byte is ever written.
 * Any pitch, offset and pointer alignment is accepted (byte accesses).  The vector path -- dword / 8-byte Y groups, an interleaved
 * chroma row loaded ONCE for both planes (the aligned centre pair-of-pairs as one dword or one 8-byte load, each outer column as one
 * 2-byte or dword load: three loads per chroma row where two planes take six), both planes' chroma of a lane stored as one dword or
 * one 8-byte store -- runs when the pointers are aligned as for the calls above, pitch is a multiple of 4 bytes, interleaved chroma has
 * chroma_pitch and chroma_offset multiples of 4 bytes (planar chroma: of 2 samples), and W, x0, w, Wp, pad_left are multiples of 4.
 * Both paths give the same bits.  Every output byte is written by exactly one lane; vector stores only, no atomics, nothing
 * pre-zeroed.  All checks run on the host before the launch (ATMVFI_EINVAL).
 * A decoder's surface that already lies in device memory (rocDecode, VA-API / AMF interop) is decoded in place:
 * hand over the mapped pointer with the surface's pitch and chroma offset; nothing is repacked or copied.
 *
 * Planar 4:2:2 and 4:4:4 frames, 8 and 10 bit (atm-vfi_amd/yuv.py: Format.subsampling; per-pixel model tests/cpu_yuv_sub.py):
 *   subsampling    0: 4:2:0, chroma planes [(H + 1) / 2, (W + 1) / 2]; 1: 4:2:2, chroma planes [H, (W + 1) / 2]; 2: 4:4:4, chroma
 *                  planes [H, W].  Planes are Y, U, V in that order, as in I420.
 * Depth 8 and 10 have the sample types, coefficients, yo, mid, T, range rules and clips of the calls above; no new coefficient exists.
 * Decode 4:2:2: chroma row r = y (no vertical filter); the columns q0, q1 and the weights (wx0, wx1) are those of 4:2:0 for both
 *   sitings; c' = (wx0 c[y][q0] + wx1 c[y][q1] + 2) >> 2.  Decode 4:4:4: c' = c[y][x].  The pixel from (Y, U', V') is unchanged for both
 *   pixel maxima (clip8 and q / 255; keep_depth: 0..1023 and q / 1023).
 * Encode: the source pixel p and Y are unchanged; chroma from the un-rounded sums s -- 4:2:2 centre: over columns 2i and
 *   min(2i + 1, W - 1) of row j, sh = 1; 4:2:2 left: max(2i - 1, 0), 2i, min(2i + 1, W - 1) weighted 1, 2, 1, sh = 2; 4:4:4: s = p,
 *   sh = 0 -- U = clip(((eU . s + 2^(13 + sh)) >> (14 + sh)) + mid), V with eV.
 * Identities that hold bit for bit (from (4 h + 8) >> 4 == (h + 2) >> 2 and (2 x + 2^(k+1)) >> (k+1) == (x + 2^k) >> k): a 4:2:2 frame
 *   whose chroma rows are all equal decodes to the pixels of the 4:2:0 frame that holds those rows; flat U and V planes decode to the same
 *   pixels under all three subsamplings; a picture whose rows 2j and 2j + 1 are equal has 4:2:2 chroma rows 2j equal to the 4:2:0 encode's
 *   row j; with columns 2i and 2i + 1 equal and centre siting the 4:4:4 chroma at column 2i is the 4:2:2 sample i.
 * The window origin must be a multiple of the subsampling step per axis: 4:2:0 even y0 and x0, 4:2:2 even x0 and any y0, 4:4:4 any.
 *   Chroma neighbours clamp at the FRAME's edges, never at the window's.  pitch / chroma_pitch / chroma_offset follow the rules above with
 *   the chroma row width cw b and H chroma rows per plane; the planar V plane follows U at chroma_offset + chroma_pitch * H.
 * Refused on the host before any launch (ATMVFI_EINVAL), in addition to what a 4:2:0 surface refuses: an unknown subsampling;
 *   interleaved chroma (chroma != 0) or msb with subsampling != 0; siting 1 with 4:4:4 (it has no meaning there); a window origin that
 *   breaks the rule above.
 * Any geometry, pitch and pointer alignment is accepted (byte accesses).  The vector path runs under the conditions of the surfaces;
 *   for 4:4:4 the chroma rows must be dword-aligned like the luma rows (chroma_pitch and the U / V origins multiples of 4 bytes).  A lane
 *   owns four horizontally adjacent pixels on two rows; 4:2:2 loads one chroma row per luma row (two per lane, no vertical mix), 4:4:4
 *   loads U and V of a group as it loads Y (a dword, or 8 bytes at depth 10); the encode stores a lane's chroma per plane and row as a
 *   2-byte or dword pair (4:2:2) or a dword or 8 bytes (4:4:4).  Both paths give the same bits.  Every output byte is written by exactly
 *   one lane; vector stores only, no atomics, nothing pre-zeroed; no padding byte is ever written.
 * Not covered: 12 bit, 4:1:1 / 4:4:0, interleaved or packed 4:2:2 / 4:4:4 (NV16, P210, YUY2, UYVY, Y210, AYUV, Y410), alpha, bt2020 and
 *   transfer functions, the area mode (mode 1) on anything but a packed planar LSB 4:2:0 frame.
 *
 * THE FRAME DESCRIPTOR (ABI 0.29).  Everything above about one frame -- its size, its samples, its colour and where the samples lie --
 * is one block without pointers, which a caller builds once per stream and passes by address to atmvfi_yuv_decode, atmvfi_yuv_encode,
 * atmvfi_yuv_compose and atmvfi_yuv_borders (a launch plan holds it by address, as the other blocks).  Fields are only ever appended
 * and zero means default / off (as atmvfi_gemm_params): a zeroed block plus H, W, depth and matrix is the tight packed planar
 * limited-range centre-sited 4:2:0 frame (I420).  The pointers, the window and the canvas of a call stay positional.
 * atmvfi_yuv_decode: `mode` 0 crop / 1 area 2x (above); keep_depth 0 / 1; without dst the output geometry is the window's.
 * atmvfi_yuv_encode: the destination is the TIGHT frame of the descriptor: pitch, chroma_pitch and chroma_offset are not read. */
typedef struct atmvfi_yuv_desc {
    int32_t H, W;               /* luma size, >= 1, odd sizes allowed */
    int32_t depth;              /* 8: uint8 samples; 10: little-endian uint16, values 0..1023 */
    int32_t matrix;             /* 0 bt601, 1 bt709 */
    int32_t full_range;         /* 0 limited, 1 full (depth 8 only) */
    int32_t siting;             /* 0 centre ("420jpeg"), 1 left ("420mpeg2"); 0 for 4:4:4 */
    int32_t subsampling;        /* 0 4:2:0, 1 4:2:2, 2 4:4:4 (1, 2: planar, LSB) */
    int32_t chroma;             /* 0 planar U then V, 1 interleaved U first (NV12, P010), 2 interleaved V first (NV21) */
    int32_t msb;                /* depth 10: a stored sample is value << 6 (P010) */
    int64_t pitch;              /* bytes between luma rows; 0: tight */
    int64_t chroma_pitch;       /* bytes between chroma rows; 0: tight */
    int64_t chroma_offset;      /* byte offset of the first chroma row; 0: pitch * H */
} atmvfi_yuv_desc;
int atmvfi_yuv_decode(const atmvfi_yuv_desc* desc, const void* yuv, int keep_depth, int mode, int y0, int x0, int h, int w, void* dst_u8,
                      int bgr, float* dst, int Hp, int Wp, int pad_top, int pad_left, void* stream);
int atmvfi_yuv_encode(const atmvfi_yuv_desc* desc, const void* src_u8, int bgr, const float* src, int Hp, int Wp, int pad_top, int pad_left,
                      void* yuv, void* stream);

/* Packed 4:2:2 capture frames (yuv_packed.hip; ABI 0.23; atm-vfi_amd/pixfmt.py: Packed; host twins yuv.unpack_numpy / pack_numpy;
 * per-sample model tests/cpu_yuv_packed.py).  Nothing of the reference.  Two sample-exact moves -- shifts and masks only -- between a
 * packed frame and `planar`, the tight planar 4:2:2 frame of the layout's depth: Y [H,W], U [H,W/2], V [H,W/2] back to back, uint8 or
 * little-endian uint16 with the value in the low bits: what atmvfi_yuv_decode / atmvfi_yuv_encode (subsampling 1) read and write.
 *   layout  depth  packed samples  memory order per pixel pair                                      default pitch (bytes)
 *   0 uyvy    8    uint8           U0 Y0 V0 Y1                                                      2 W
 *   1 yuy2    8    uint8           Y0 U0 Y1 V0                                                      2 W
 *   2 y210   10    uint16 (LE)     Y0 U0 Y1 V0, each sample value << 6 (read s >> 6, written v << 6) 4 W
 *   3 v210   10    bytes           groups of four LE 32-bit words for 6 pixels, see below           ((W + 47) / 48) * 128
 *   A v210 word holds three components in bits 0-9, 10-19 and 20-29; bits 30-31 are zero:
 *     w0 = (Cb0, Y0, Cr0)   w1 = (Y1, Cb1, Y2)   w2 = (Cr1, Y3, Cb2)   w3 = (Y4, Cr2, Y5);   Cb_k / Cr_k belong to pixels 2k and 2k + 1.
 *   W is even (every layout carries chroma per pixel pair).  pitch: the packed rows' stride in bytes, at least the row's own bytes
 *   (2 W, 2 W, 4 W, ceil(W / 6) * 16) and a multiple of 4 (v210: 16); 0: the default.
 * Padding rule.  Bytes and component slots of a packed frame that hold no sample -- a row's bytes beyond its samples up to the pitch,
 *   v210's component slots beyond W in the last group, v210's bits 30-31, y210's low six bits -- are NEVER INTERPRETED by unpack (no
 *   byte beyond a row's own bytes is read at all) and WRITTEN AS ZERO by pack, which writes every byte of the default-pitch frame
 *   (pitch * H) itself and never reads `packed`.  Planar samples are values of the depth (pack drops higher bits: v & 1023 for v210,
 *   (v << 6) mod 2^16 for y210).
 * atmvfi_yuv_unpack: packed (at `pitch`) -> planar, every planar sample written.  atmvfi_yuv_pack: planar -> packed at the DEFAULT pitch.
 * Refused on the host before any launch (ATMVFI_EINVAL): null pointers; H < 1, W < 2 or W odd; an unknown layout; a pitch that is
 *   negative, short or no multiple of 4 (v210: 16); a base pointer that is not sample-aligned (packed v210: 4-byte aligned); overlapping
 *   packed and planar ranges; a work-item count that does not fit an int.
 * Any other geometry and alignment is accepted.  Aligned path (both pointers 16-byte aligned, the pitch a multiple of 16; layouts 0-2:
 *   W a multiple of 16 / the sample size; v210: W a multiple of 8): 16-byte accesses of the packed row, 16-byte accesses of the luma
 *   row and 8-byte accesses of the chroma rows; a v210 lane owns four whole groups (64 packed bytes, 48 + 24 + 24 planar bytes), the
 *   groups behind a row's last whole four -- the partial last group among them -- and pack's zero groups of the padding go one per
 *   lane through dword and sample accesses, as every group does on the general path.  Both paths give the same bits.  One launch,
 *   grid-stride, every output byte written by exactly one lane: vector stores only, no atomics, nothing pre-zeroed. */
int atmvfi_yuv_unpack(const void* packed, int H, int W, int layout, int64_t pitch /*0: default*/, void* planar, void* stream);
int atmvfi_yuv_pack(const void* planar, int H, int W, int layout, void* packed /*default pitch*/, void* stream);

/* Deep RGB frames, 10 / 12 / 16 bit (rgb16.hip; ABI 0.25; atm-vfi_amd/pixfmt.py: DeepRGB; host twins atm-vfi_amd/rgb16.py; per-sample model
 * tests/cpu_rgb16.py).  Nothing of the reference, whose scripts read 8-bit images.  A frame is tight: 3 H W little-endian uint16 samples,
 * LSB-aligned, top = 2^depth - 1.
 *   layout 0 rgb48 : interleaved R G B (the bytes of a uint16 [H,W,3] array)
 *   layout 1 bgr48 : interleaved B G R
 *   layout 2 gbrp  : three planes [H,W] in the order G, B, R (ffmpeg's gbrp10le / gbrp12le / gbrp16le)
 * atmvfi_rgb16_decode.  q' = min(q, top): bits above the depth are never trusted.  The window (y0, x0, h, w) of the frame, any origin, as
 *   dst, fp32 planar RGB [3,Hp,Wp] = q' / top with the bits of the fp32 division (atmvfi_frame_u8_to_f32's pixel with top in place of
 *   255), the window at (pad_top, pad_left), replicate padding of the window's own edge pixels -- and / or dst_u8, the frame's 8-bit
 *   PROBE picture uint8 [h,w,3] RGB = q' >> (depth - 8), on which atmvfi_frame_signature and atmvfi_frame_difference run unchanged (cut
 *   and duplicate decisions are those of the 8-bit picture obtained by truncation).  Without dst, Hp / Wp / pad_* are not read.
 * atmvfi_rgb16_encode.  p = clip(rint(fl32(x * top)), 0, top), half to even, of the H x W picture at (pad_top, pad_left) of src (finite
 *   values; outside [0, 1] they clamp; atmvfi_frame_f32_to_u8's pixel with top in place of 255), written in the layout's order; nothing
 *   of src outside the picture is read.  rint(fl32(fl32(q / top) * top)) == q for every code of the three depths, and at depth 16 the
 *   decode of q = 257 b is fl32(b / 255), atmvfi_frame_u8_to_f32's value for b.
 * Refused on the host before any launch (ATMVFI_EINVAL): a null source (encode: a null destination); decode with both outputs NULL; a
 *   depth other than 10, 12, 16; an unknown layout; sizes below 1; a window outside the frame; a canvas that does not hold the picture
 *   plus padding; a frame pointer that is not 2-byte or a canvas pointer that is not 4-byte aligned; a work-item count beyond 2^30.
 * Any other geometry and alignment is accepted.  A lane owns four adjacent pixels of a row (decode: of the padded canvas, so padding is
 *   written by the lanes that own it).  Aligned path -- the frame 8-byte aligned, W % 4 == 0 (decode: x0 % 4 == 0 and w % 4 == 0 too), the
 *   canvas 16-byte aligned with Wp % 4 == 0 and pad_left % 4 == 0, dst_u8 4-byte aligned: one 16-byte access per fp32 plane, three 8-byte
 *   accesses of an interleaved frame (gbrp: one per plane), three dwords of the probe picture.  General path: 2-byte accesses of the frame
 *   and scalar accesses of the canvas.  Both give the same bits.  One launch, grid-stride, every output byte written by exactly one
 *   lane: vector stores only, no atomics, nothing pre-zeroed, no LDS. */
int atmvfi_rgb16_decode(const void* src, int H, int W, int depth, int layout, int y0, int x0, int h, int w,
                        float* dst /*[3,Hp,Wp] or NULL*/, int Hp, int Wp, int pad_top, int pad_left,
                        void* dst_u8 /*[h,w,3] RGB or NULL*/, void* stream);
int atmvfi_rgb16_encode(const float* src /*[3,Hp,Wp]*/, int Hp, int Wp, int pad_top, int pad_left,
                        void* dst, int H, int W, int depth, int layout, void* stream);

/* mean |a - b| per sample: global_alignmentness (network_base.py:560-561).  Two passes with a fixed summation order -- the result is
 * run-to-run bit-identical (the ensemble's pick compares these means) -- through `workspace`: at least
 * atmvfi_l1_mean_workspace_floats(B, per_sample) floats of scratch, the caller's. */
int64_t atmvfi_l1_mean_workspace_floats(int B, int64_t per_sample);
int atmvfi_l1_mean(const float* a, const float* b, float* out, int B, int64_t per_sample, float* workspace, int64_t workspace_floats, void* stream);
/* multiscale_global_motion_ensemble's per-sample pick (network_base.py:591-603): out0 / out1 [B, per_sample] = the candidate flow pair
 * (c0_lL, c1_lL, already at the level-0 flow resolution) of the level whose loss[b] is the minimum, the first one on ties (the
 * reference's min() / if / elif chain, NaN losses included: a NaN loss of level 0 falls through to level 2).  Keeps the ensemble forward free of device arithmetic outside this ABI. */
int atmvfi_ensemble_select(const float* loss0, const float* loss1, const float* loss2, const float* c0_l0, const float* c1_l0,
                           const float* c0_l1, const float* c1_l1, const float* c0_l2, const float* c1_l2, float* out0, float* out1, int B,
                           int64_t per_sample, void* stream);

/* The encoder's full-resolution stem in one launch: feat_extracts.0.0 (3 -> C0, 3x3 + PReLU), feat_extracts.0.1 (C0 -> C0, 3x3 + PReLU) and
 * feat_extracts.1.0 (C0 -> C1, 3x3 stride 2 + PReLU) of shared_feat_extraction (network_base.py:99-110, 342-352), (C0, C1) = (24, 48) or
 * (16, 32).  x: the NHWC4-packed frames [F, H, W, 4] (atmvfi_pack_frames), H and W even.  The two full-resolution C0-channel maps never
 * leave the chip (LDS); the result is written as split planes (chunk-major, out_plane_rows >= F * H/2 * W/2 rows per 32-channel chunk),
 * rows = pixels (f, y, x) of the half-resolution map.  All three layers use the f16x3 split (x = hi + lo'/1024, three 16-bit MFMAs per
 * product, fp32 accumulation).  Weights as the host packs them (atm-vfi_amd/hip_ops.py::HipOps.pack_stem), fp16 hi / lo' planes:
 *   w1 [round_up(C0, 16)][32], k = (ky * 3 + kx) * 3 + ci (27 values, then zeros);  w2 [NS][round_up(C0, 16)][32] and w3 [NS][C1][32],
 *   NS = ceil(9 C0 / 32) k-steps of 32 k-values, k = (ky * 3 + kx) * C0 + c, zero beyond 9 C0 and in padded rows;
 *   b1 / p1 and b2 / p2 [round_up(C0, 16)] (bias 0, slope 1 in the padding), b3 / p3 [C1]: bias and PReLU slope of each layer. */
int atmvfi_stem_fused(const float* x, int F, int H, int W, int C0, int C1, const void* w1_hi, const void* w1_lo, const float* b1, const float* p1,
                      const void* w2_hi, const void* w2_lo, const float* b2, const float* p2, const void* w3_hi, const void* w3_lo,
                      const float* b3, const float* p3, void* out_hi, void* out_lo, int64_t out_plane_rows, void* stream);

/* ------------------------------------------------------------------------------------
 * Quality metrics (metrics.hip): ssim_matlab of the reference's evaluation scripts (benchmark/pytorch_msssim.py:82-135: an 11x11x11
 * Gaussian conv3d over channels, H and W on replicate-padded inputs) and the squared-error mean of PSNR, for B frame pairs at once.
 *   x: the reference's img1 (the ground truth): fp32, or uint8 with ATMVFI_SSIM_X_U8 (then x = (float)u / 255.0f, and channel c is
 *      read from channel 2 - c with ATMVFI_SSIM_X_BGR); y: fp32.  Both are [B,3,H,W] views given by element strides (batch, channel,
 *      row, column), so an un-padded slice or a uint8 HWC frame (strides H*W*3, 1, W*3, 3) is read in place.
 *   val_range > 0: the L of C1 = (0.01 L)^2, C2 = (0.03 L)^2; otherwise the reference's rule on x, applied on the device
 *      (max > 128 -> 255 else 1, minus min < -0.5 -> -1 else 0), over all B samples as torch.max(img1) does.
 *   ATMVFI_SSIM_ROUND_Y: y is replaced by rint(y * 255) / 255 in fp32 first (UCF101 protocol).
 *   mse: mean of (x - y)^2 accumulated in fp64; the difference and square in fp64 (u8: u / 255.0 in double), in fp32 with
 *      ATMVFI_SSIM_MSE_F32.
 *   out: fp64 [B,3] = (ssim, cs, mse) per sample, written, or added to with ATMVFI_SSIM_ACCUMULATE (a running sum over a dataset).
 * H, W >= 11 (the reference shrinks its window below that: not supported, ATMVFI_EINVAL).  Scratch: at least
 * atmvfi_ssim_psnr_workspace_floats(B, H, W) floats, 16-byte aligned, the caller's.  Fixed reduction order, no float atomics: two runs
 * are bit-identical. */
#define ATMVFI_SSIM_X_U8 1
#define ATMVFI_SSIM_X_BGR 2
#define ATMVFI_SSIM_ROUND_Y 4
#define ATMVFI_SSIM_ACCUMULATE 8
#define ATMVFI_SSIM_MSE_F32 16
#define ATMVFI_SSIM_FLAG_MASK 31
int64_t atmvfi_ssim_psnr_workspace_floats(int B, int H, int W);
int atmvfi_ssim_psnr(const void* x, int64_t x_bstride, int64_t x_cstride, int64_t x_ystride, int64_t x_xstride, const float* y,
                     int64_t y_bstride, int64_t y_cstride, int64_t y_ystride, int64_t y_xstride, int B, int H, int W, float val_range,
                     int flags, double* out, float* workspace, int64_t workspace_floats, void* stream);

/* Interlaced input (fields.hip; ABI 0.27; the definitions, the host twins and the loop: atm-vfi_amd/fields.py; per-pixel models:
 * tests/cpu_fields.py).  Nothing of the reference.  Neither call is part of a forward.
 * atmvfi_field_bob.  src [planes,Hp,Wp] fp32 is a WOVEN canvas whose picture S is the h x w window at (pad_top, pad_left); per plane and
 *   parity p the bobbed picture is
 *       F_p[y] = S[y] if (y & 1) == p;  else S[1] if y == 0;  else S[h-2] if y == h-1;  else 0.5f * (S[y-1] + S[y+1])
 *   (the fp32 sum rounded once, the halving exact), and the field canvas the network reads is the replicate padding of the BOBBED picture:
 *       dst_p[c][Y][X] = F_p[c][clamp(Y - pad_top, 0, h-1)][clamp(X - pad_left, 0, w-1)]
 *   dst_even takes p = 0 and dst_odd p = 1, both [planes,Hp,Wp]; either may be NULL, not both.  One launch reads the picture once and
 *   writes both: a lane owns four adjacent canvas columns of a strip of ATMVFI_FIELD_BOB_STRIP picture rows and keeps the previous two
 *   source rows in registers.  16-byte accesses when the three pointers are 16-byte aligned and Wp, pad_left and w are multiples of 4,
 *   scalar accesses otherwise; the same bits.  The source's padding is never read; every element of a destination is written by
 *   exactly one lane; vector stores only, no atomics, nothing pre-zeroed, no host synchronisation.
 *   ATMVFI_EINVAL before any launch: a null source or two null destinations, planes < 1, h < 2, w < 1, a window outside the canvas, a
 *   destination that overlaps the source or the other destination.
 * atmvfi_field_rows.  Per plane k (geometry[6k..6k+5] = dst_offset, src_offset, dst_pitch, src_pitch, row_bytes, rows; bytes; a HOST
 *   array read at the call, its values travel in the kernel arguments): for every row y < rows with (y & 1) == parity, the row_bytes
 *   bytes at src + src_offset + y * src_pitch replace those at dst + dst_offset + y * dst_pitch.  Bytes are moved, nothing is
 *   computed; rows of the other parity and bytes beyond row_bytes are neither read nor written.  A plane whose two base addresses, two
 *   pitches and row_bytes are multiples of 16 moves 16 bytes per lane, any other plane single bytes; the same bits.
 *   ATMVFI_EINVAL before any launch: a null pointer, planes outside 1..3, a parity outside 0 / 1, a negative offset, a pitch,
 *   row_bytes or rows below 1, row_bytes above a pitch, rows written that overlap rows read or the rows written of another plane. */
#define ATMVFI_FIELD_BOB_STRIP 16
int atmvfi_field_bob(const float* src /*[planes,Hp,Wp]*/, float* dst_even, float* dst_odd, int planes, int Hp, int Wp, int pad_top, int pad_left,
                     int h, int w, void* stream);
int atmvfi_field_rows(void* dst, const void* src, int planes /*1..3*/,
                      const int64_t* geometry /*HOST array, 6 per plane: dst_offset, src_offset, dst_pitch, src_pitch, row_bytes, rows*/, int parity,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * Launch plans: one forward of the hot path as ONE call.
 *
 * The reference's callers run `model(im0, im1)` in a loop on frames of one size (benchmark/test_vimeo90k.py: 3 782 triplets of
 * 256x448; demo_2x.py:129-168: every pair of a video).  For such a loop the sequence of launches of a forward is fixed: same entry
 * points, same arguments, except the pointers into the caller's two frames and into the freshly allocated output tensors.  The host
 * records that sequence once (every launch entry point above, arguments in declaration order, stream excluded) and replays it:
 * atmvfi_plan_run() first patches the arguments that point into per-call memory -- ops[p.op].a[p.arg] = slots[p.slot] + p.offset --
 * and then issues the ops in order on `stream`, stopping at the first failure (*failed_op = its index; the return value and
 * atmvfi_last_error() are that op's).  Nothing is cached inside the library: the plan is the caller's array.
 * atmvfi_plan_fn_id(name) gives the `fn` of an entry point by name (-1 if it is not a launch entry point).
 *
 * Host integer lists.  atmvfi_pool_blocks takes its slot list as a HOST array: a recorded op holds that array's address, and the
 * entry point reads, validates (range, duplicates of a scatter) and copies the `n` values into the kernel arguments at LAUNCH time,
 * i.e. inside atmvfi_plan_run().  This is a contract: the owner of a plan may rewrite the values of such an array between two
 * atmvfi_plan_run() calls (its address and length are fixed by the recording) and each replay moves the slots named at that moment;
 * nothing of an earlier replay is remembered.  The array must stay alive as long as the plan, like a parameter block.
 * ---------------------------------------------------------------------------------- */
typedef union atmvfi_plan_arg { uint64_t u; int64_t i; double f; } atmvfi_plan_arg;
#define ATMVFI_PLAN_MAX_ARGS 28
typedef struct atmvfi_plan_op {
    int32_t fn;       /* atmvfi_plan_fn_id() */
    int32_t nargs;    /* must equal the entry point's argument count without the stream (checked) */
    atmvfi_plan_arg a[ATMVFI_PLAN_MAX_ARGS];   /* pointers and sizes as .u / .i (64-bit), float arguments as .f */
} atmvfi_plan_op;
typedef struct atmvfi_plan_patch { int32_t op, arg, slot, reserved; int64_t offset; } atmvfi_plan_patch;
int atmvfi_plan_fn_id(const char* name);
int atmvfi_plan_run(atmvfi_plan_op* ops, int n_ops, const atmvfi_plan_patch* patches, int n_patches, const uint64_t* slots, int n_slots,
                    int* failed_op, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ATMVFI_H */
