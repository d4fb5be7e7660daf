// Device primitives shared by the HIP kernels of this directory: the vector typedefs, the fp16 / bf16 element traits with
// the 16x16x32 MFMA of the type, nn.GELU, the XCD tile order, the LDS-DMA and its wait, the software bf16 conversions and
// the quad DPP helpers.  One definition of each: a kernel source includes this header and declares none of them itself.
//
// Everything sits in an anonymous namespace, the one the kernels themselves live in: every name is internal to the
// translation unit that includes the header (no ODR question between objects built with different flags), a kernel uses
// the names unqualified, and the mangled name of a kernel template instantiated on a trait stays
// `(anonymous namespace)::kernel<(anonymous namespace)::HalfT, ...>`, which the plan exporter's name matcher expects.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- software bfloat16 <-> fp32 on raw bits: round to nearest even as ATen does, a NaN stays a (quiet) NaN.  The small
// kernels that are tested bit for bit against ATen use these; the GEMM epilogues use the hardware converter (BFloatT).
__device__ __forceinline__ float bf16_to_f32(unsigned short bits) { return __uint_as_float(((unsigned)bits) << 16); }
__device__ __forceinline__ unsigned short bf16_from_f32(float v) {
  const unsigned u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// ---- ReLU on eight packed 16-bit floats, x < 0 ? 0 : x with a NaN of either sign kept (the contract of every epilogue;
// v_pk_max_f16(x, 0) returns 0 for a NaN, v_pk_max_i16(x, 0) for a NaN with the sign bit set).  Sign-magnitude floats
// read as int16: the negative numbers, -0 and -inf are exactly the values <= kNegInf (the bits of -inf), the NaNs with the
// sign bit set lie above it.  kNegInf - x (saturating) is negative exactly for the values to keep: arithmetic shift, and --
// three packed operations per two values; -0 -> +0.
template <class F, short kNegInf>
__device__ __forceinline__ F relu_bits16(F x) {
  s16x8 i;
  __builtin_memcpy(&i, &x, 16);
  u32x4 keep = __builtin_bit_cast(u32x4, __builtin_elementwise_sub_sat((s16x8)kNegInf, i) >> 15);
  asm("" : "+v"(keep));   // (keeps the mask a mask: the compiler otherwise rewrites this as a compare + select per value)
  i = __builtin_bit_cast(s16x8, __builtin_bit_cast(u32x4, i) & keep);
  __builtin_memcpy(&x, &i, 16);
  return x;
}

// ---- element types: fp16 / bf16 storage, fp32 accumulation on the matrix cores either way
struct HalfT {
  using elem = _Float16;
  using frag = f16x8;
  using v4 = f16x4;
  __device__ static f32x4 mfma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
  __device__ static float to_f32(unsigned short bits) {
    _Float16 h;
    __builtin_memcpy(&h, &bits, 2);
    return (float)h;
  }
  __device__ static unsigned short from_f32(float v) {
    _Float16 h = (_Float16)v;
    unsigned short bits;
    __builtin_memcpy(&bits, &h, 2);
    return bits;
  }
  // two fp32 -> one dword of two halves (round to nearest even: v_cvt_pk_f16_f32 on gfx950)
  __device__ static unsigned pack2(float lo, float hi) {
    f16x2 h = {(_Float16)lo, (_Float16)hi};
    unsigned o;
    __builtin_memcpy(&o, &h, 4);
    return o;
  }
  __device__ static s16x4 pack4(const float (&v)[4]) {  // 2 x v_cvt_pk_f16_f32
    f16x4 h = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    s16x4 o;
    __builtin_memcpy(&o, &h, 8);
    return o;
  }
  __device__ static frag relu(frag x) { return relu_bits16<frag, (short)0xfc00>(x); }
};
struct BFloatT {
  using elem = __bf16;
  using frag = bf16x8;
  using v4 = bf16x4;
  __device__ static f32x4 mfma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
  __device__ static float to_f32(unsigned short bits) { return bf16_to_f32(bits); }
  // fp32 -> bf16 on the hardware converter (v_cvt_pk_bf16_f32, round to nearest even, NaN stays quiet): the 5-instruction
  // integer rounding made every bf16 epilogue ~30 vector instructions per 4 outputs longer than its fp16 twin
  __device__ static unsigned short from_f32(float v) {
    const __bf16 h = (__bf16)v;
    return __builtin_bit_cast(unsigned short, h);
  }
  __device__ static unsigned pack2(float lo, float hi) {
    const bf16x2 h = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned, h);
  }
  __device__ static s16x4 pack4(const float (&v)[4]) {
    const bf16x4 h = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    return __builtin_bit_cast(s16x4, h);
  }
  __device__ static frag relu(frag x) { return relu_bits16<frag, (short)0xff80>(x); }
};

// ---- nn.GELU (erf form): 0.5 x (1 + erf(x / sqrt 2)).  libm's erff costs ~50 VALU ops per element and made the GELU
// epilogues VALU-bound; erf is evaluated with Abramowitz-Stegun 7.1.26 instead (|erf error| <= 1.5e-7).
//   0.5 x (1 + erf(x / sqrt 2)) = 0.5 x + |x| (0.5 - (0.5 p(t) t) exp(-x^2 / 2)),  t = 1 / (1 + 0.3275911 |x| / sqrt 2):
// the sign of erf folds into |x|, the halves into the coefficients -- 11 plain operations + v_rcp + v_exp.
// What that is worth (tests/test_epilogue_exact_cpu.py emulates the formula over every fp16 / bf16 input, the GPU test
// runs it through the kernels): the error is ABSOLUTE, at most 2.4e-7 |x| for the formula in fp32 and at most 4.8e-7 |x|
// with the two 1-ulp hardware operations -- far below the fp16 / bf16 rounding of the result wherever |gelu(x)| is of
// the order of |x|, but not a relative bound: for -6 < x < -3 the fp16 result is up to 2 ulp from the correctly rounded
// one, and in the far tail (x < -5, |gelu(x)| < 1e-6) the relative error reaches 100 % and the sign is not preserved.
__device__ __forceinline__ float gelu_erf(float x) {
  const float u = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752f, u, 1.0f));
  float p = fmaf(0.5f * 1.061405429f, t, 0.5f * -1.453152027f);
  p = fmaf(p, t, 0.5f * 1.421413741f);
  p = fmaf(p, t, 0.5f * -0.284496736f);
  p = fmaf(p, t, 0.5f * 0.254829592f);
  const float ez = __builtin_amdgcn_exp2f(u * u * (-0.5f * 1.4426950408889634f));
  return fmaf(u, fmaf(-(p * t), ez, 0.5f), 0.5f * x);
}
// the same function on two values at once: the 11 plain operations as 6 packed ones (v_pk_fma_f32 / v_pk_mul_f32 are full
// rate on gfx950 when no MFMA competes for the issue slot -- an epilogue), v_rcp / v_exp per element.  Same operations in
// the same order as gelu_erf, so the fp32 results are bit-identical.  The STORED value need not be: where gelu_erf's result
// goes straight to fp16 the compiler fuses the last fma with the conversion (v_fma_mix{lo,hi}_f16: one rounding), while
// the packed form rounds to fp32 and then to fp16 -- the last fp16 bit differs on a few inputs (4 of the 184 326 of the
// exact-epilogue test); bf16 has no such instruction and is identical.
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 x) {
  const f32x2 u = {fabsf(x.x), fabsf(x.y)};
  const f32x2 d = __builtin_elementwise_fma(f32x2{0.3275911f * 0.70710678118654752f, 0.3275911f * 0.70710678118654752f}, u,
                                            f32x2{1.0f, 1.0f});
  const f32x2 t = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  f32x2 p = __builtin_elementwise_fma(f32x2{0.5f * 1.061405429f, 0.5f * 1.061405429f}, t,
                                      f32x2{0.5f * -1.453152027f, 0.5f * -1.453152027f});
  p = __builtin_elementwise_fma(p, t, f32x2{0.5f * 1.421413741f, 0.5f * 1.421413741f});
  p = __builtin_elementwise_fma(p, t, f32x2{0.5f * -0.284496736f, 0.5f * -0.284496736f});
  p = __builtin_elementwise_fma(p, t, f32x2{0.5f * 0.254829592f, 0.5f * 0.254829592f});
  const f32x2 e = (u * u) * f32x2{-0.5f * 1.4426950408889634f, -0.5f * 1.4426950408889634f};
  const f32x2 ez = {__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
  const f32x2 h = __builtin_elementwise_fma(-(p * t), ez, f32x2{0.5f, 0.5f});
  return __builtin_elementwise_fma(u, h, x * f32x2{0.5f, 0.5f});
}

// ---- XCD-aware tile order: the hardware deals workgroups round-robin over the 8 XCDs, so blocks with equal
// (blockIdx % 8) share an L2.  Give each such group one contiguous run of tiles.  Bijective for any grid size
// (cdna_hip_programming.md T1).  Placement only affects speed.
__device__ __forceinline__ unsigned xcd_tile(unsigned bid, unsigned nblk) {
  const unsigned q = nblk >> 3, r = nblk & 7u, x = bid & 7u, i = bid >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ---- LDS-DMA: 16 B per lane (1 KiB per wave instruction) from (wave-uniform 64-bit base `src` in SGPRs) + (per-lane
// 32-bit byte offset `voff`) to the wave-uniform LDS address `lds_addr` + lane * 16.  Inline assembly, not
// __builtin_amdgcn_global_load_lds: the compiler's wait-count pass files the builtin with out-of-order LDS traffic and
// from then on turns every wait for a ds_read into lgkmcnt(0), which voids the fragment read-ahead; the instruction only
// counts in vmcnt, which the callers wait on by hand (wait_vmcnt).  M0 is written in the statement that reads it and is
// declared clobbered: the compiler may keep nothing in it across the block.
__device__ __forceinline__ void lds_dma16(const unsigned char* src, unsigned voff, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(src), "s"(lds_addr)
               : "memory", "m0");
}
__device__ __forceinline__ void lds_dma16(const unsigned char* src, unsigned voff, unsigned char* dst) {
  lds_dma16(src, voff, (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)dst));
}
// the builtin form (per-lane 64-bit source address), for the kernels that leave the wait counts to the compiler
__device__ __forceinline__ void lds_dma16_auto(const void* g, unsigned char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
// at most N vector-memory operations (LDS-DMA pieces included) of this wave still in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- floor + float -> int in one instruction
__device__ __forceinline__ int floor_i(float v) {
  int d;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(d) : "v"(v));
  return d;
}

// ---- quad (4-lane) data movement on the DPP path
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __uint_as_float(dpp_u<CTRL>(__float_as_uint(v)));
}
constexpr int kXor1 = 0xB1, kXor2 = 0x4E;  // quad_perm [1,0,3,2] / [2,3,0,1]
__device__ __forceinline__ unsigned quad_bcast_u(unsigned v, int owner) {
  switch (owner) {
    case 0: return dpp_u<0x00>(v);
    case 1: return dpp_u<0x55>(v);
    case 2: return dpp_u<0xAA>(v);
    default: return dpp_u<0xFF>(v);
  }
}
__device__ __forceinline__ float quad_bcast_f(float v, int owner) { return __uint_as_float(quad_bcast_u(__float_as_uint(v), owner)); }
// quad broadcast of `v` from lane `owner` plus this lane's `add`: ONE v_add_u32_dpp
__device__ __forceinline__ unsigned quad_bcast_add(unsigned v, int owner, unsigned add) {
  unsigned d;
  switch (owner) {
    case 0: asm("v_add_u32_dpp %0, %1, %2 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(v), "v"(add)); break;
    case 1: asm("v_add_u32_dpp %0, %1, %2 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(v), "v"(add)); break;
    case 2: asm("v_add_u32_dpp %0, %1, %2 quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(v), "v"(add)); break;
    default: asm("v_add_u32_dpp %0, %1, %2 quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(v), "v"(add)); break;
  }
  return d;
}

}  // namespace
