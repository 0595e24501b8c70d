// The colour byte of the exported cloud, shared by every kernel that writes one (cloud.hip's PLY records, render.hip's images):
// a pixel rendered from source pixel p carries the bytes that the PLY export writes for p.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint8_t cc_colour(float c) {      // host.write_ply_binary: (uint8)(clip((double)c, 0, 1) * 255)
  const double v = fmin(fmax((double)c, 0.0), 1.0) * 255.0;
  return (uint8_t)(int)v;
}
