// What the kernels that read detections share (prepost.hip, draw.hip, appearance.hip, the tracker): the element types a
// box or a score is stored in, and the library's IoU.  One definition of each, in the anonymous namespace as device_prims.h.
#pragma once
#include "device_prims.h"

namespace {

// bfloat16 storage (the bf16 model's instantiations); the conversion is exact, NaN stays NaN
struct Bf16 {
  unsigned short bits;
};
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(_Float16 v) { return (float)v; }
__device__ __forceinline__ float to_f32(Bf16 v) { return bf16_to_f32(v.bits); }

// IoU of two boxes given their areas, fp32 with one rounding per operation (no contraction into an FMA, whatever the
// including file's setting: the CPU references round w * h before they subtract); NaN for two zero-area boxes.  With
// contraction off (w * h) of the same box is the same rounded product every time it is computed, so an area may be stored
// or computed again.
__device__ __forceinline__ float box_area(float4 b) {
#pragma clang fp contract(off)
  const float w = b.z - b.x, h = b.w - b.y;
  return w * h;
}
__device__ __forceinline__ float box_iou(float4 bk, float ak, float4 bj, float aj) {
#pragma clang fp contract(off)
  const float w = fmaxf(0.f, fminf(bk.z, bj.z) - fmaxf(bk.x, bj.x));
  const float h = fmaxf(0.f, fminf(bk.w, bj.w) - fmaxf(bk.y, bj.y));
  const float inter = w * h;
  const float uni = ak + aj;
  return inter / (uni - inter);
}

}  // namespace
