// The pixel region of a detection row, shared by the kernels that act on the pixels under a box (redact.hip, crops.hip):
// the rule include/codetr_redact.h states under "Region" -- each coordinate clamped to [-16384, 16383], the box grown by
// `expand` of its width and height, floor / ceil - 1 to whole pixels.  fp32 with one rounding per operation (no
// contraction, whatever the including file's setting).  One definition, in the anonymous namespace as device_prims.h.
#pragma once
#include "device_prims.h"

namespace {

__device__ __forceinline__ float clamp_coord(float v) { return fminf(fmaxf(v, -16384.f), 16383.f); }

// the region (X1, Y1, X2, Y2), both ends inclusive and not yet clipped to an image; false when it does not exist
__device__ __forceinline__ bool region_of(float x1, float y1, float x2, float y2, float expand, int4* r) {
#pragma clang fp contract(off)
  x1 = clamp_coord(x1), y1 = clamp_coord(y1), x2 = clamp_coord(x2), y2 = clamp_coord(y2);
  const float w = x2 - x1, h = y2 - y1;
  const float ex = expand * w, ey = expand * h;
  const float a1 = clamp_coord(x1 - ex), a2 = clamp_coord(x2 + ex);
  const float b1 = clamp_coord(y1 - ey), b2 = clamp_coord(y2 + ey);
  *r = make_int4((int)floorf(a1), (int)floorf(b1), (int)ceilf(a2) - 1, (int)ceilf(b2) - 1);
  return r->z >= r->x && r->w >= r->y;
}

}  // namespace
