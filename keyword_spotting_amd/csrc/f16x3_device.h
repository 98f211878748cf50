// "f16x3" operand arithmetic shared by gru_f16x3.hip, gru_f16x3_generic.hip and attention_f16x3.hip: a value travels as two fp16
// pieces, v = hi + lo with hi = fp16(v) (both round-to-nearest-even), and a product takes three v_mfma_f32_16x16x32_f16.
// Two conventions for lo, which must not be mixed within one product:
//   scaled     lo = fp16((v - hi) 2^11), in an accumulator of its own that is folded in with kLoInv: never an fp16 subnormal
//   unscaled   lo = fp16(v - hi), into the same accumulator as hi: for hidden values, |v| <= 1 (gru_f16x3.hip's header)
#pragma once
#include <hip/hip_runtime.h>

namespace kws {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr float kLoScale = 2048.f, kLoInv = 1.f / 2048.f;
constexpr float kMelScale = 1.f / 256.f;       // the packed x-part weights of a first layer / the embedding are multiplied by 256
constexpr float kHalfMax = 65504.f;

__device__ __forceinline__ f16x8 as_f16x8(u32x4 v) { return __builtin_bit_cast(f16x8, v); }
__device__ __forceinline__ f32x4 mfma_f16(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_f16(u32x4 a, u32x4 b, f32x4 c) { return mfma_f16(as_f16x8(a), as_f16x8(b), c); }

__device__ __forceinline__ float clamp_half(float v) { return __builtin_fminf(__builtin_fmaxf(v, -kHalfMax), kHalfMax); }
// two values -> their packed hi and 2^11-scaled lo pieces
__device__ __forceinline__ void split2(f32x2 x, unsigned& hi, unsigned& lo) {
    const f16x2 h = __builtin_convertvector(x, f16x2);
    const f32x2 r = (x - __builtin_convertvector(h, f32x2)) * kLoScale;
    const f16x2 l = __builtin_convertvector(r, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ void split1(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)((x - (float)hi) * kLoScale);
}
// hidden values (|v| <= 1): lo UNSCALED
__device__ __forceinline__ void split2u(f32x2 x, unsigned& hi, unsigned& lo) {
    const f16x2 h = __builtin_convertvector(x, f16x2);
    const f32x2 r = x - __builtin_convertvector(h, f32x2);
    const f16x2 l = __builtin_convertvector(r, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
// Two C tiles -> one chunk of the next B operand, (hi, lo).  Two functions on purpose: the unscaled lo of split8_unscaled goes into
// the accumulator of hi (gru_f16x3.hip), the scaled lo of split8_scaled into a lo accumulator (gru_f16x3_generic.hip).
__device__ __forceinline__ void split8_unscaled(const f32x4& a, const f32x4& b, u32x4& hi, u32x4& lo) {
    unsigned h[4], l[4];
    split2u((f32x2){a[0], a[1]}, h[0], l[0]);
    split2u((f32x2){a[2], a[3]}, h[1], l[1]);
    split2u((f32x2){b[0], b[1]}, h[2], l[2]);
    split2u((f32x2){b[2], b[3]}, h[3], l[3]);
    hi = (u32x4){h[0], h[1], h[2], h[3]};
    lo = (u32x4){l[0], l[1], l[2], l[3]};
}
__device__ __forceinline__ void split8_scaled(const f32x4& a, const f32x4& b, u32x4& hi, u32x4& lo) {
    unsigned h[4], l[4];
    split2((f32x2){a[0], a[1]}, h[0], l[0]);
    split2((f32x2){a[2], a[3]}, h[1], l[1]);
    split2((f32x2){b[0], b[1]}, h[2], l[2]);
    split2((f32x2){b[2], b[3]}, h[3], l[3]);
    hi = (u32x4){h[0], h[1], h[2], h[3]};
    lo = (u32x4){l[0], l[1], l[2], l[3]};
}
// four mel values of a first layer: scale by 2^-8, clamp to fp16's range (larger magnitudes saturate), split; (hi, lo) as the two
// dword pairs the B-operand image takes
__device__ __forceinline__ void mel_split4(f32x4 mel, uint2& hi, uint2& lo) {
    f32x4 v = mel * kMelScale;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = clamp_half(v[e]);
    unsigned h0, l0, h1, l1;
    split2((f32x2){v[0], v[1]}, h0, l0);
    split2((f32x2){v[2], v[3]}, h1, l1);
    hi = make_uint2(h0, h1);
    lo = make_uint2(l0, l1);
}

}  // namespace
}  // namespace kws
