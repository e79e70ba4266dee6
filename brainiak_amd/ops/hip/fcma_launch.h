// Everything fcma_kernels.hip exports, declared once.  The kernels file
// includes this header, so its definitions are checked against it; the
// Torch binding includes it instead of keeping a copy.
//
// The launchers that map a runtime (P, L) onto a template instantiation
// return int: 1 when a kernel was launched, 0 when (P, L) has no
// instantiation and nothing was launched.
#pragma once

#include <hip/hip_runtime_api.h>

extern "C" {
// shape envelope
long long fcma_supported_L(long long L);   // L padded up, -1 if too long
int fcma_corr_norm_smem(long long L, int P);
int fcma_corr_norm_z8_supported(long long E, int P, long long L);
int fcma_fused_gram_supported(long long E, int P, long long L);
long long fcma_duo_gram_blocks(long long Cg, long long Eg,
                               long long nsplit);

// correlation (+ normalize)
void launch_fcma_normalize(float* corr, long long C, long long E,
                           long long V, int P, hipStream_t stream);
int launch_fcma_corr_norm(const void* A, const void* B, void* zOut,
                          float* fOut, long long E, long long L,
                          long long VA, long long VB, long long s0,
                          long long C, int P, int mode, long long zstride,
                          hipStream_t stream, const void* At);
int launch_fcma_corr_raw(const void* At, const void* B, void* zOut,
                         long long E, long long L, long long VB,
                         long long C, long long zstride, int P,
                         hipStream_t stream);
int launch_fcma_corr_norm_z8(const void* At, const void* B, void* zOut,
                             long long E, long long L, long long VB,
                             long long C, long long zstride, int P,
                             hipStream_t stream);
int launch_fcma_corr_gram_duo(
    const void* At, const void* B, void* zOut, long long E, long long L,
    long long VB, long long C, long long zstride, int P,
    const void* Zprev, float* G, long long Cg, long long Eg, long long Vg,
    long long nsplit, const float* GpSum, float* GSumOut, long long Cs,
    long long nsplitSum, int do_shrink, hipStream_t stream);
int launch_fcma_fused_corr_gram(const void* A, const void* B,
                                float* Gpart, long long L, long long VA,
                                long long VB, long long s0, long long C,
                                int nsplit, hipStream_t stream);

// Gram
void launch_fcma_gram_bf16(const void* Z, float* G, long long C,
                           long long E, long long V, long long nsplit,
                           hipStream_t stream);
void launch_fcma_gram_bf16_norm(const void* Z, float* G, long long C,
                                long long E, long long V,
                                long long nsplit, int P,
                                hipStream_t stream);
void launch_fcma_gram_fp8(const void* Z, float* G, long long C,
                          long long E, long long V, long long nsplit,
                          hipStream_t stream);
void launch_fcma_gram_f32(const float* Z, float* G, long long C,
                          long long E, long long V, hipStream_t stream);
void launch_fcma_gsum(const float* Gp, float* Gout, long long Cs,
                      long long EE, long long nsplit, int do_shrink,
                      hipStream_t stream);

// fp8 conversion probes
void launch_fp8_cvt_probe(const float* x, void* o, long long n,
                          hipStream_t stream);
void launch_fp8_cvt_probe_sw(const float* x, void* o, long long n,
                             hipStream_t stream);
}
