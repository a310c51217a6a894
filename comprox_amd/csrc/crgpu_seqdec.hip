/*
 * comprox_amd/csrc/crgpu_seqdec.hip — the kernels of crgpu_seqdec.h (many sequences of dependent comprop, comprox or comprolz
 * blocks decoded in one launch) as a translation unit of their own, and their launchers; the host side of the feature is in crgpu.hip.
 */
#include <hip/hip_runtime.h>

#define CRGPU_SEQDEC_TU
#include "crgpu_seqdec.h"

static_assert(CR_V5_LDS_BYTES == 272u + 256u * (CR_V5_DLDS + 1u) && CRGPU_NODE_WORDS == 64u, "the k_seqdec kernels refill the dense nodes' LDS copies at word 68 + 64 k");

void crsd_launch_mark(hipStream_t s, uint8_t* store, u64 stride, const uint32_t* which, uint32_t n) {
    hipLaunchKernelGGL(k_seqdec_mark, dim3((n + 255u) / 256u), dim3(256), 0, s, store, stride, which, n);
}
void crsd_launch_decode(hipStream_t s, int which, uint32_t grid, const CrSeqDec& D, const CrArenaLayout& L) {
    if (which == CR_SD_ROX) hipLaunchKernelGGL(k_seqdec_rox_v5, dim3(grid), dim3(CRGPU_WAVE), 0, s, D, L);
    else if (which == CR_SD_ROLZ) hipLaunchKernelGGL(k_seqdec_rolz_v5, dim3(grid), dim3(CRGPU_WAVE), 0, s, D, L);
    else hipLaunchKernelGGL(k_seqdec_v5, dim3(grid), dim3(CRGPU_WAVE), 0, s, D, L);
}
const void* crsd_decode_kernel(int which) {
    return which == CR_SD_ROX ? reinterpret_cast<const void*>(k_seqdec_rox_v5) : which == CR_SD_ROLZ ? reinterpret_cast<const void*>(k_seqdec_rolz_v5)
                                                                                                    : reinterpret_cast<const void*>(k_seqdec_v5);
}
const char* crsd_decode_name(int which) { return which == CR_SD_ROX ? "k_seqdec_rox_v5" : which == CR_SD_ROLZ ? "k_seqdec_rolz_v5" : "k_seqdec_v5"; }
