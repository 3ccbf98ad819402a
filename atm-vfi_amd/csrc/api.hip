// Error reporting and version of libatmvfi_hip.so.
#include "common.h"

#include <string.h>

#include <vector>

namespace atmvfi {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return ATMVFI_ELAUNCH;
    }
    return ATMVFI_OK;
}

#ifdef ATMVFI_RANGE_CHECK
static std::vector<RangeWordSetter>& range_registry() {
    static std::vector<RangeWordSetter> v;      // (function-local: filled by other translation units' static initialisers)
    return v;
}
void range_registry_add(RangeWordSetter s) { range_registry().push_back(s); }
#endif

}  // namespace atmvfi

extern "C" int atmvfi_range_word_set(uint32_t* word, void* stream) {
#ifdef ATMVFI_RANGE_CHECK
    for (atmvfi::RangeWordSetter set : atmvfi::range_registry()) {
        const int e = set(reinterpret_cast<unsigned*>(word), (hipStream_t)stream);
        ATMVFI_REQUIRE(e == 0, ATMVFI_ELAUNCH, "range_word_set: hipMemcpyToSymbolAsync failed (%d)", e);
    }
    return ATMVFI_OK;
#else
    (void)word; (void)stream;
    atmvfi::set_error("range_word_set: this is the default build; the operand range check lives in libatmvfi_hip_checked.so (make checked)");
    return ATMVFI_EINVAL;
#endif
}
extern "C" int atmvfi_range_checked(void) {
#ifdef ATMVFI_RANGE_CHECK
    return 1;
#else
    return 0;
#endif
}

extern "C" int atmvfi_version(void) { return (0 << 16) | (29 << 8) | 0; }   // 0.29: atmvfi_yuv_decode / atmvfi_yuv_encode on the frame descriptor atmvfi_yuv_desc replace the nine positional YUV conversion entry points; atmvfi_yuv_compose and atmvfi_yuv_borders take the descriptor; 0.28: atmvfi_conv3p on atmvfi_conv3p_params replaces the six positional entry points of the 3x3 plane kernel (`out` = the first stored channel; the read-out is a mode of the call); 0.27: atmvfi_field_bob, atmvfi_field_rows (interlaced input; fields.hip); 0.26: atmvfi_frame_half, atmvfi_synth_up2, atmvfi_synth_up2_workspace_floats (half-resolution motion; warp.hip); 0.25: atmvfi_rgb16_decode, atmvfi_rgb16_encode (deep RGB frames, 10 / 12 / 16 bit; rgb16.hip); 0.24: ATMVFI_PREC_F16 and a term count for the 3x3 plane kernel and its read-out (the single-pass fp16 mode of the plane kernels); 0.23: atmvfi_yuv_unpack, atmvfi_yuv_pack (packed 4:2:2: uyvy, yuy2, y210, v210; yuv_packed.hip); 0.22: atmvfi_yuv_borders, atmvfi_yuv_compose (active.hip, yuv_encode.hip); 0.21: atmvfi_frame_borders, atmvfi_frame_compose (active.hip); 0.20: planar 4:2:2 / 4:4:4 decode and encode (yuv.hip, yuv_encode.hip); 0.19: decoder-surface decode and encode (NV12 / NV21 / P010, pitched; yuv.hip, yuv_encode.hip); 0.18: atmvfi_shutter_accumulate, atmvfi_shutter_resolve, atmvfi_shutter_table (shutter.hip); 0.17: the YUV window decode with the area mode (yuv_window.hip); 0.16: atmvfi_frame_difference (framediff.hip); 0.15: 10-bit YUV 4:2:0 with the depth kept (yuv10.hip); 0.14: YUV 4:2:0 <-> RGB (yuv.hip); 0.13: atmvfi_frame_signature (scene.hip); 0.12: atmvfi_pool_blocks, atmvfi_tta_merge, atmvfi_frame_rot180; 0.11: atmvfi_frame_u8_window; 0.10: launch plans run on one stream (the lanes entry point and its record / wait ops removed); 0.9: atmvfi_flow_warp_ex, atmvfi_range_word_set / atmvfi_range_checked (the checked build); 0.8: atmvfi_source_digest; 0.7: atmvfi_window_attention_f16x3, compact fp32 view behind out_cmin of the 3x3 plane kernel, saturating conversions by MODE.FP16_OVFL; 0.6: 3x3 kernel on split-plane input, plane sinks and CONV mode of the LDS-DMA GEMM, per-call instance overrides (no process-wide state); 0.5: plane sink of the 3x3 kernel; 0.4: split-plane sinks, k-step-major planes, uint8 frame kernels
extern "C" const char* atmvfi_last_error(void) { return atmvfi::g_err; }
#ifndef ATMVFI_SOURCE_DIGEST
#define ATMVFI_SOURCE_DIGEST "unknown (api.hip compiled outside the Makefile)"
#endif
extern "C" const char* atmvfi_source_digest(void) { return ATMVFI_SOURCE_DIGEST; }
