/*
 * comprox_amd/csrc/crgpu_dictset.hip — the kernels of crgpu_dictset.h (the tries of a dictionary set, built on the device) as a
 * translation unit of their own, and their launchers; the host side of the feature is in crgpu.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crgpu_device.h"
#define CRGPU_DICTSET_TU
#include "crgpu_dictset.h"

void crds_launch_sort(hipStream_t s, const CrDictSetBuild& P) { hipLaunchKernelGGL(k_dset_sort, dim3(P.ndict), dim3(CRDS_THREADS), 0, s, P); }
void crds_launch_link(hipStream_t s, const CrDictSetBuild& P) { hipLaunchKernelGGL(k_dset_link, dim3(P.ndict), dim3(CRDS_THREADS), 0, s, P); }
void crds_launch_mark(hipStream_t s, const CrDictSetBuild& P, uint32_t max_words) {
    hipLaunchKernelGGL(k_dset_mark, dim3((max_words + 255u) / 256u, P.ndict), dim3(256), 0, s, P);
}
void crds_launch_ids(hipStream_t s, const CrDictSetBuild& P, uint32_t grid_x) { hipLaunchKernelGGL(k_dset_ids, dim3(grid_x, P.ndict), dim3(256), 0, s, P); }
void crds_launch_finish(hipStream_t s, const CrDictSetBuild& P, uint32_t grid_x) { hipLaunchKernelGGL(k_dset_finish, dim3(grid_x, P.ndict), dim3(256), 0, s, P); }
