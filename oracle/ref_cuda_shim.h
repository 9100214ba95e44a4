// Force-included (-include) in front of the reference's four CUDA kernel files when
// oracle/ref_build.py compiles them with hipcc for gfx950.  Name mappings only: the CUDA
// runtime spellings those files use, onto their HIP equivalents.  No kernel code lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>  // nms_cuda_kernel.cu calls memset without including it

#define cudaError_t hipError_t
#define cudaSuccess hipSuccess
#define cudaStream_t hipStream_t
#define cudaGetErrorString hipGetErrorString
#define cudaGetLastError hipGetLastError
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaMalloc hipMalloc
#define cudaFree hipFree
#define cudaMemcpy hipMemcpy
#define cudaMemcpyHostToDevice hipMemcpyHostToDevice
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
