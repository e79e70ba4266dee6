// Shared device helpers for the FCMA HIP kernels (gfx950): vector
// typedefs, the bf16 MFMA fragment map and the scale-free Fisher z.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64
typedef __hip_bfloat16 bf16_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
// 4-byte-aligned variant for global loads: gfx950 dwordx4 loads need
// only dword alignment, and bf16 rows are 4B- but not 16B-aligned
typedef short bf16x8_u __attribute__((ext_vector_type(8), aligned(4)));
typedef long long ll;

// ---------------------------------------------------------------------------
// MFMA fragment maps, v_mfma_f32_16x16x32_bf16 (gfx950):
//   A (16x32): lane l, j in 0..7 -> A[l%16][frag_k(l,j)]
//   B (32x16): lane l, j in 0..7 -> B[frag_k(l,j)][l%16]
//   C/D (16x16, f32x4): col = lane&15, row = (lane>>4)*4 + reg
// frag_k isolated so a layout flip is one line, guarded by GPU numerics
// tests (tests/ops/test_hip_ops.py::test_gram_identity_asymmetric).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int frag_k(int lane, int j) {
    return 8 * (lane >> 4) + j;
}

// scale-free Fisher z: log2(num) - log2(den).  The downstream
// within-subject z-score (z - mean) * rsqrt(var) is invariant to the
// 0.5*ln2 factor, so the kernels that always z-score skip the multiply
// (one VALU op per element on an issue-bound kernel).
__device__ __forceinline__ float fisher_z_unscaled(float r) {
    float num = 1.0f + r;
    float den = 1.0f - r;
    num = (num <= 0.0f) ? 1e-4f : num;
    den = (den <= 0.0f) ? 1e-4f : den;
    return __builtin_amdgcn_logf(num) - __builtin_amdgcn_logf(den);
}

// fisher_z_unscaled for an r that has just been rounded to bf16.  Next
// to +-1 the bf16 grid is 2^-8 wide, so 1 +- r is either <= 0 or at
// least 2^-8: max(x, 1e-4) then picks exactly what the compare-and-
// select clamp picks (checked over all 65536 bf16 values) at half the
// VALU instructions.
__device__ __forceinline__ float fisher_z_unscaled_bf16r(float r) {
    float num = __builtin_fmaxf(1.0f + r, 1e-4f);
    float den = __builtin_fmaxf(1.0f - r, 1e-4f);
    return __builtin_amdgcn_logf(num) - __builtin_amdgcn_logf(den);
}
