/*
 * comprox_amd/csrc/crgpu_carry.hip — the kernels of crgpu_carry.h (comprop's chain encoder on carried models) as a
 * translation unit of their own, and their launchers; the host side of the feature is in crgpu.hip.
 */
#include <hip/hip_runtime.h>

#define CRGPU_CARRY_TU
#include "crgpu_carry.h"

void crc_launch_fill(hipStream_t s, uint32_t grid, uint8_t* M) { hipLaunchKernelGGL(k_ropc_fill, dim3(grid), dim3(256), 0, s, M); }
void crc_launch_events(hipStream_t s, const CrBatch& B1, const CrArenaLayout& L, uint8_t* M) { hipLaunchKernelGGL(k_ropc_events, dim3(1), dim3(CRGPU_WAVE), 0, s, B1, L, M); }
void crc_launch_o3(hipStream_t s, uint32_t grid, const CrBatch& B1, uint8_t* M) { hipLaunchKernelGGL(k_ropc_o3, dim3(grid), dim3(256), 0, s, B1, M); }
void crc_launch_o2(hipStream_t s, uint32_t grid, const CrBatch& B1, uint8_t* M) { hipLaunchKernelGGL(k_ropc_o2, dim3(grid), dim3(CR_O2C_THREADS), 0, s, B1, M); }
void crc_launch_o1(hipStream_t s, const CrBatch& B1, uint8_t* M) { hipLaunchKernelGGL(k_ropc_o1, dim3(1), dim3(CR_O1_THREADS), 0, s, B1, M); }
void crc_launch_abort(hipStream_t s, const CrBatch& B1, uint8_t* M) { hipLaunchKernelGGL(k_ropc_abort, dim3(1), dim3(CRGPU_WAVE), 0, s, B1, M); }
