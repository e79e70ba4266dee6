// FCMA HIP/CDNA4 kernels for MI355X (gfx950).
//
// MI355X-native re-design of the reference's FCMA native layer:
//  - ref src/brainiak/fcma/cython_blas.pyx:20-116  (per-epoch sgemm)  -> k_corr_norm
//  - ref src/brainiak/fcma/src/fcma_extension.cc:29-86 (OpenMP norm)  -> k_normalize / fused
//  - ref src/brainiak/fcma/cython_blas.pyx:118-207 (per-voxel ssyrk)  -> k_gram_bf16 (MFMA) / k_gram_f32
//
// Design (per /opt/skills/guides/cdna_hip_programming.md):
//  * wave64, 256-thread blocks.
//  * The correlation+normalization stage ships the two variants that won
//    their measurements (profiles/README.md has the ladder and the
//    losers' numbers): dot3s (thread owns all P epochs of a column, the
//    wave-uniform A operand on the SCALAR path — no LDS, no barriers)
//    for bf16 Z with P in {2,4}, and dot2 (v_dot2c_f32_bf16 + fused
//    normalize/store) for everything else.  launch_corr_norm_t holds
//    that rule; dispatch_pl maps a runtime (P, L) onto the templates.
//  * k_gram_bf16: G_c = Z_c Z_c^T via v_mfma_f32_16x16x32_bf16, T14
//    issue-early K-tiles, V-split partials so small-C calls fill the
//    256 CUs.  k_fused_corr_gram: the whole chunk in one kernel
//    (opt-in; measured slower than the streamed pipeline — see notes).
//  * epochs_per_subj is a template parameter for the common values so
//    per-column z[] arrays stay in registers (runtime-indexed arrays
//    drop to scratch - guide rule 20); a generic two-pass path covers
//    the rest.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <iterator>
#include <type_traits>
#include <utility>

#include "fcma_common.h"
#include "fcma_launch.h"

// --- fp8 (OCP e4m3fn) Z-tile path -----------------------------------------
// The normalized Z values are within-subject z-scores, bounded by
// sqrt(P-1) (<= 1.74 for the headline P=4), so e4m3's 3-bit mantissa
// (~3 % RMS quantization) is the only loss; the Gram accumulates in
// fp32 MFMA.  Halves the Z HBM round trip (profiles/NEXT.md item 1).
#include <hip/amd_detail/amd_hip_fp8.h>
typedef unsigned char fp8_t;
typedef unsigned int uint32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ fp8_t to_fp8(float v) {
    __hip_fp8_e4m3 t(v);
    return t.__x;
}

// store-cast for the corr kernel's templated output type
template <typename OT>
__device__ __forceinline__ OT z_cast(float v);
template <>
__device__ __forceinline__ bf16_t z_cast<bf16_t>(float v) {
    return (bf16_t)v;
}
template <>
__device__ __forceinline__ fp8_t z_cast<fp8_t>(float v) {
    return to_fp8(v);
}

__device__ __forceinline__ float fisher_z(float r) {
    float num = 1.0f + r;
    float den = 1.0f - r;
    num = (num <= 0.0f) ? 1e-4f : num;   // reference clamp semantics
    den = (den <= 0.0f) ? 1e-4f : den;
    // raw v_log_f32 (log2), no denormal fixup: the clamp bounds the
    // arguments to [1e-4, 2], far from the denormal range — __logf's
    // ~10-instruction range-check chain is dead weight here (PMC: the
    // normalize stage was the largest VALU block of the corr kernel)
    const float half_ln2 = 0.34657359028f;   // 0.5 * ln(2)
    return half_ln2 * (__builtin_amdgcn_logf(num)
                       - __builtin_amdgcn_logf(den));
}

// ===========================================================================
// k_normalize: standalone in-place Fisher-z + within-subject z-score of
// corr [C, E, V] fp32.  One thread per (c, subject, v) column.
// ===========================================================================
template <int TP>
__global__ __launch_bounds__(256) void k_normalize(
    float* __restrict__ corr, ll C, ll E, ll V, int Prt) {
    const int P = TP > 0 ? TP : Prt;
    const ll nSubj = E / P;
    const ll vBlocks = (V + 255) / 256;
    ll b = blockIdx.x;
    const ll vb = b % vBlocks; b /= vBlocks;
    const ll s = b % nSubj;    b /= nSubj;
    const ll c = b;
    const ll v = vb * 256 + threadIdx.x;
    if (c >= C || v >= V) return;

    float* col = corr + (c * E + s * (ll)P) * V + v;
    if (TP > 0) {
        float z[TP > 0 ? TP : 1];
        float mean = 0.f, sq = 0.f;
        #pragma unroll
        for (int p = 0; p < P; ++p) {
            z[p] = fisher_z(col[(ll)p * V]);
            mean += z[p]; sq += z[p] * z[p];
        }
        mean /= (float)P;
        float var = sq / (float)P - mean * mean;
        float inv = (var <= 0.f) ? 0.f : rsqrtf(var);
        #pragma unroll
        for (int p = 0; p < P; ++p)
            col[(ll)p * V] = (z[p] - mean) * inv;
    } else {
        float mean = 0.f, sq = 0.f;
        for (int p = 0; p < P; ++p) {
            float zv = fisher_z(col[(ll)p * V]);
            mean += zv; sq += zv * zv;
        }
        mean /= (float)P;
        float var = sq / (float)P - mean * mean;
        float inv = (var <= 0.f) ? 0.f : rsqrtf(var);
        for (int p = 0; p < P; ++p)
            col[(ll)p * V] = (fisher_z(col[(ll)p * V]) - mean) * inv;
    }
}

// ===========================================================================
// The corr kernels: fused correlation + normalization for one
// (voxel-tile, subject, column-tile):
//   corr[c,p,v] = sum_k A[s*P+p, k, s0+c0+c] * B[s*P+p, k, v0+v]
//   out        = zscore_p(fisher_z(corr))        (modes 0/1)
// A: [E, L, VA] bf16, B: [E, L, VB] bf16 (stacked z-scored epochs; zero
// padding rows are inert).  mode 0: bf16 Z out; 2: fp32 RAW correlation
// out (no normalization).  The launchers pass nothing else: the kernels'
// mode 1 (fp32 normalized out) and mode 3 (write-skip probe) branches
// are dead and stay only so that the generated code does not move.
// TL = compile-time epoch length (the host pads epochs to a supported
// length with zero rows) so the per-thread B column stays in registers
// with fully unrolled dot chains.
// ===========================================================================
#define CN_CT 16
#define CN_VT 64

// ===========================================================================
// k_corr_norm_dot2: the v_dot2c_f32_bf16 form of the corr stage.
// ISA evidence for the pk_fma kernel it replaced (77 s_waitcnt per 64
// ds_read_b128 + 128 v_pk_fma_f32 in the unrolled k-loop, fp32 A tile,
// 16-voxel c-tile): the wave stalls on nearly
// every LDS read and pays 8 b128 broadcasts per 32 MACs.  Here the A tile
// stays bf16 (its source dtype) in k-pair-interleaved layout
// [p][k/2][c][2], so one ds_read_b128 feeds FOUR c-columns x k-pair and
// one v_dot2c_f32_bf16 retires TWO MACs with exact f32 accumulation —
// half the LDS bytes AND half the VALU issue of the pk_fma form — and
// the next k-pair's A quads are register-staged while the current pair
// is dotted (T14), so each k-step carries one batched s_waitcnt.
// ===========================================================================
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef short short2_t __attribute__((ext_vector_type(2)));

template <int TP, int TL>
__global__ __launch_bounds__(256) void k_corr_norm_dot2(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ zOut, float* __restrict__ fOut,
    ll E, ll Lrt, ll VA, ll VB, ll s0, ll C, int Prt, int mode,
    ll zstride) {
    static_assert(TL % 2 == 0, "dot2 corr kernel requires even L");
    // c-tile width: every B element is register-reused across TCT
    // selected voxels, so LLC/HBM B traffic scales as 1/TCT; bounded by
    // LDS (corr tile TCT*P*VT fp32) and VGPRs (acc[TCT])
    // measured on MI355X: TCT=64 (72 KB LDS -> 8 waves/CU) halves the
    // corr floor's occupancy and regresses 2x despite 4x less B traffic
    // - the kernel needs ~16+ waves/CU to hide the B-column load
    // latency.  TCT=32 (36 KB -> 16 waves/CU) is the measured optimum.
    constexpr int TCT = (TP > 0 && TP <= 4) ? 32 : CN_CT;
    const int P = TP > 0 ? TP : Prt;
    const ll L = TL;
    (void)Lrt;
    const ll nSubj = E / P;
    const ll cTiles = (C + TCT - 1) / TCT;
    const ll vTiles = (VB + CN_VT - 1) / CN_VT;
    ll b = blockIdx.x;
    const ll vt = b % vTiles; b /= vTiles;
    const ll s = b % nSubj;   b /= nSubj;
    const ll ct = b;
    if (ct >= cTiles) return;

    const ll c0 = ct * TCT;
    const ll v0 = vt * CN_VT;
    const int CT = (int)min((ll)TCT, C - c0);
    const int VT = (int)min((ll)CN_VT, VB - v0);
    const int tid = threadIdx.x;

    extern __shared__ char smem[];
    // a_tile [P][L/2][TCT][2] bf16 (k-pair interleaved), corr fp32
    bf16_t* a_tile = (bf16_t*)smem;
    float* corr = (float*)(a_tile + (size_t)P * TL * TCT);
    constexpr int KP = TL / 2;

    for (int idx = tid; idx < P * (int)L * TCT; idx += 256) {
        int c = idx % TCT;
        int k = (idx / TCT) % (int)L;
        int p = idx / (TCT * (int)L);
        bf16_t val = (bf16_t)0.0f;
        if (c < CT)
            val = A[((s * P + p) * L + k) * VA + (s0 + c0 + c)];
        a_tile[(((size_t)p * KP + (k >> 1)) * TCT + c) * 2 + (k & 1)]
            = val;
    }
    __syncthreads();

    for (int base = tid; base < P * CN_VT; base += 256) {
        int v = base % CN_VT;
        int p = base / CN_VT;
        if (v < VT) {
            // b column as bf16 k-pairs (kept in source dtype)
            bf16x2_t bp[KP];
            const bf16_t* brow = B + ((ll)(s * P + p) * L) * VB + (v0 + v);
            #pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                bf16x2_t t;
                t[0] = *(const __bf16*)&brow[(ll)(2 * kp) * VB];
                t[1] = *(const __bf16*)&brow[(ll)(2 * kp + 1) * VB];
                bp[kp] = t;
            }
            float acc[TCT];
            #pragma unroll
            for (int c = 0; c < TCT; ++c) acc[c] = 0.f;
            // explicit ds_read_b128 of 4 c-pairs; the scheduler runs the
            // reads several k-pairs ahead with counted lgkmcnt waits
            // (verified in the ISA) — no manual pipeline needed
            const bf16x8* arow8 = (const bf16x8*)
                (a_tile + ((size_t)p * KP) * TCT * 2);
            #pragma unroll
            for (int kp = 0; kp < KP; ++kp)
                #pragma unroll
                for (int q = 0; q < TCT / 4; ++q) {
                    bf16x8 raw = arow8[kp * (TCT / 4) + q];
                    #pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        short2_t s2 = {raw[2 * j], raw[2 * j + 1]};
                        acc[4 * q + j] = __builtin_amdgcn_fdot2_f32_bf16(
                            __builtin_bit_cast(bf16x2_t, s2), bp[kp],
                            acc[4 * q + j], false);
                    }
                }
            #pragma unroll
            for (int c = 0; c < TCT; ++c)
                corr[((size_t)c * P + p) * CN_VT + v] = acc[c];
        }
    }
    __syncthreads();

    if (mode == 2) {
        for (int base = tid; base < CT * P * CN_VT; base += 256) {
            int v = base % CN_VT;
            int p = (base / CN_VT) % P;
            int c = base / (CN_VT * P);
            if (v < VT)
                fOut[((c0 + c) * E + (s * P + p)) * VB + v0 + v] =
                    corr[((size_t)c * P + p) * CN_VT + v];
        }
        return;
    }

    // normalization FUSED with the output store: one thread per (c, v)
    // column; z stays in registers between fisher_z and the
    // (lane-coalesced) store — no corr writeback, no re-read pass, one
    // barrier fewer than the classic kernel
    for (int base = tid; base < CT * CN_VT; base += 256) {
        int v = base % CN_VT;
        int c = base / CN_VT;
        if (v >= VT) continue;
        float* col = corr + ((size_t)c * P) * CN_VT + v;
        float mean = 0.f, sq = 0.f;
        if (TP > 0) {
            float z[TP > 0 ? TP : 1];
            #pragma unroll
            for (int p = 0; p < P; ++p) {
                z[p] = fisher_z(col[(size_t)p * CN_VT]);
                mean += z[p]; sq += z[p] * z[p];
            }
            mean /= (float)P;
            float var = sq / (float)P - mean * mean;
            float inv = (var <= 0.f) ? 0.f : rsqrtf(var);
            if (mode == 0) {
                bf16_t* dst = zOut
                    + ((c0 + c) * zstride + s * (ll)P) * VB + v0 + v;
                #pragma unroll
                for (int p = 0; p < P; ++p)
                    dst[(size_t)p * VB] = (bf16_t)((z[p] - mean) * inv);
            } else if (mode == 3) {
                // write-skip PROBE (bounds the fused-kernel gain): the
                // never-true predicate keeps the compute alive
                #pragma unroll
                for (int p = 0; p < P; ++p)
                    if (zstride < 0)
                        zOut[(size_t)tid] =
                            (bf16_t)((z[p] - mean) * inv);
            } else {
                float* dst = fOut
                    + ((c0 + c) * E + s * (ll)P) * VB + v0 + v;
                #pragma unroll
                for (int p = 0; p < P; ++p)
                    dst[(size_t)p * VB] = (z[p] - mean) * inv;
            }
        } else {
            for (int p = 0; p < P; ++p) {
                float zv = fisher_z(col[(size_t)p * CN_VT]);
                mean += zv; sq += zv * zv;
            }
            mean /= (float)P;
            float var = sq / (float)P - mean * mean;
            float inv = (var <= 0.f) ? 0.f : rsqrtf(var);
            for (int p = 0; p < P; ++p) {
                float zv = (fisher_z(col[(size_t)p * CN_VT]) - mean)
                           * inv;
                if (mode == 0)
                    zOut[((c0 + c) * zstride + (s * P + p)) * VB
                         + v0 + v] = (bf16_t)zv;
                else
                    fOut[((c0 + c) * E + (s * P + p)) * VB + v0 + v] =
                        zv;
            }
        }
    }
}

// ===========================================================================
// k_corr_norm_dot3s: thread-owns-all-epochs form (P <= 4) with the A
// operand read through the SCALAR path.
// The dot2 kernel's (chalf,p,v)->normalize->(c,v) split forces the fp32
// corr tile through LDS (the 4 epochs of one (c,v) column live in 4
// different waves).  Here ONE thread owns (v, all P epochs): it dots,
// Fisher-z's, z-scores and stores each c's column entirely in
// registers.  Every lane of a wave reads the same a-pair (c and s are
// wave-uniform), so the A tile belongs in SGPRs via the constant
// cache, not in LDS: the host passes At = A[:, :, start:start+count]
// transposed to [count, E, L] (contiguous per voxel), and the kernel
// needs NO LDS, NO staging loop and NO barrier at all.
// ===========================================================================
#define C3_VT 256

template <int TP, int TL, int C3_CT, typename OT = bf16_t,
          bool RAW = false>
__device__ __forceinline__ void dot3s_body(
    ll b,
    const bf16_t* __restrict__ At, const bf16_t* __restrict__ B,
    OT* __restrict__ zOut, ll E, ll VB,
    ll C, int mode, ll zstride) {
    static_assert(TL % 2 == 0 && TP >= 2 && TP <= 4,
                  "dot3s kernel: even L, P in {2,4}");
    constexpr int P = TP;
    constexpr int KP = TL / 2;
    constexpr int L = TL;
    const ll nSubj = E / P;
    const ll cTiles = (C + C3_CT - 1) / C3_CT;
    const ll vTiles = (VB + C3_VT - 1) / C3_VT;
    const ll vt = b % vTiles; b /= vTiles;
    const ll s = b % nSubj;   b /= nSubj;
    const ll ct = b;
    if (ct >= cTiles) return;
    const ll c0 = ct * C3_CT;
    const int CT = (int)min((ll)C3_CT, C - c0);
    const ll v = vt * (ll)C3_VT + threadIdx.x;
    if (v >= VB) return;

    bf16x2_t bp[P][KP];
    #pragma unroll
    for (int p = 0; p < P; ++p) {
        const bf16_t* brow = B + ((ll)(s * P + p) * L) * VB + v;
        #pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            bf16x2_t t;
            t[0] = *(const __bf16*)&brow[(ll)(2 * kp) * VB];
            t[1] = *(const __bf16*)&brow[(ll)(2 * kp + 1) * VB];
            bp[p][kp] = t;
        }
    }

    // wave-uniform A base for this (c-tile, subject)
    const unsigned int* abase = (const unsigned int*)
        (At + (c0 * (ll)E + s * (ll)P) * L);
    const int cstride = (E * L) / 2;          // dwords per voxel

    for (int c = 0; c < CT; ++c) {
        const unsigned int* ac = abase + (ll)c * cstride;
        float acc[P];
        #pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = 0.f;
        #pragma unroll
        for (int kp = 0; kp < KP; ++kp)
            #pragma unroll
            for (int p = 0; p < P; ++p)
                acc[p] = __builtin_amdgcn_fdot2_f32_bf16(
                    __builtin_bit_cast(bf16x2_t,
                                       ac[p * (L / 2) + kp]),
                    bp[p][kp], acc[p], false);
        if (RAW) {
            // raw-correlation store: Fisher-z + z-score are deferred
            // to the Gram kernel's staging phase (whose waves sit in
            // memory-latency shadow) — this kernel is VALU-issue bound
            OT* dst = zOut
                + ((c0 + c) * zstride + s * (ll)P) * VB + v;
            #pragma unroll
            for (int p = 0; p < P; ++p)
                dst[(size_t)p * VB] = z_cast<OT>(acc[p]);
            continue;
        }
        float z[P];
        float mean = 0.f, sq = 0.f;
        #pragma unroll
        for (int p = 0; p < P; ++p) {
            z[p] = fisher_z_unscaled(acc[p]);
            mean += z[p]; sq += z[p] * z[p];
        }
        mean /= (float)P;
        float var = sq / (float)P - mean * mean;
        float inv = (var <= 0.f) ? 0.f : rsqrtf(var);
        if (mode == 3) {
            #pragma unroll
            for (int p = 0; p < P; ++p)
                if (zstride < 0)
                    zOut[(size_t)threadIdx.x] =
                        z_cast<OT>((z[p] - mean) * inv);
        } else {
            OT* dst = zOut
                + ((c0 + c) * zstride + s * (ll)P) * VB + v;
            #pragma unroll
            for (int p = 0; p < P; ++p)
                dst[(size_t)p * VB] = z_cast<OT>((z[p] - mean) * inv);
        }
    }
}

template <int TP, int TL, int C3_CT, typename OT = bf16_t,
          bool RAW = false>
__global__ __launch_bounds__(256) void k_corr_norm_dot3s(
    const bf16_t* __restrict__ At, const bf16_t* __restrict__ B,
    OT* __restrict__ zOut, ll E, ll VB,
    ll C, int mode, ll zstride) {
    dot3s_body<TP, TL, C3_CT, OT, RAW>(blockIdx.x, At, B, zOut, E, VB,
                                       C, mode, zstride);
}

// ===========================================================================
// k_fused_corr_gram: the WHOLE chunk pipeline in one kernel for the
// headline shape (E = 64 epochs, P = 4 epochs/subject):
//   corr -> Fisher-z -> z-score -> per-voxel [64,64] Gram (MFMA),
// with the normalized Z living ONLY in LDS.  Probe evidence
// (profiles/README.md): the two-kernel pipeline pays ~7.3 ms/step for
// Z's HBM round trip (bf16 write + Gram re-read, 36 GB/step); here the
// per-(c-tile, v-window) Z tile is produced in LDS and immediately
// rank-64-updated into per-wave MFMA accumulators, so HBM traffic per
// step drops to B reads (MALL-cached) + the 64 MB Gram output.
//
// Structure: 512-thread workgroup (8 waves) owns FG_CB=8 selected
// voxels; grid = c-tiles x nsplit v-ranges; each workgroup loops its
// v-windows (VT=64):
//   per subject s: stage A-pairs -> dot2 corr (thread = (chalf,p,v))
//     -> fused normalize writing bf16 z into z_smem[c][epoch][v]
//   after 16 subjects: wave w rank-updates G_{c0+w} from z_smem[w]
//     (16 MFMA tiles x 2 k-steps, same fragment map as k_gram_bf16).
// Gram accumulators persist in VGPRs across the whole v-range; the
// [nsplit, C, 64, 64] partials are summed on the host when nsplit > 1.
// ===========================================================================
#define FG_CB 8
#define FG_VT 64
#define FG_ROW 68   // bf16 z row stride: 136 B spreads the 16-lane
                    // fragment groups across banks (see LDS table)

template <int TL>
__global__ __launch_bounds__(512) void k_fused_corr_gram(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
    float* __restrict__ Gpart, ll VA, ll VB, ll s0, ll C, int nsplit) {
    static_assert(TL % 2 == 0, "fused kernel requires even L");
    constexpr int P = 4, E = 64, NSUBJ = 16, KP = TL / 2;
    const ll cTiles = (C + FG_CB - 1) / FG_CB;
    const ll vTiles = (VB + FG_VT - 1) / FG_VT;
    const ll vs = blockIdx.x % nsplit;
    const ll ct = blockIdx.x / nsplit;
    if (ct >= cTiles) return;
    const ll c0 = ct * FG_CB;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;                   // 8 waves

    __shared__ bf16_t z_smem[FG_CB][E][FG_ROW];
    __shared__ float corr_s[FG_CB][P][FG_VT];
    __shared__ bf16_t a_sm[P][KP][FG_CB][2];

    // symmetric accumulation: only the 10 upper tiles (i <= j) live in
    // registers; the lower triangle is mirrored at the store
    f32x4 G[10];
    #pragma unroll
    for (int t = 0; t < 10; ++t) G[t] = (f32x4)0.f;

    for (ll vt = vs; vt < vTiles; vt += nsplit) {
        const ll v0 = vt * FG_VT;
        for (int s = 0; s < NSUBJ; ++s) {
            // --- stage A k-pairs for this subject's 4 epochs
            for (int idx = tid; idx < P * TL * FG_CB; idx += 512) {
                int i2 = idx & 1;
                int c = (idx >> 1) % FG_CB;
                int kp = ((idx >> 1) / FG_CB) % KP;
                int p = (idx >> 1) / (FG_CB * KP);
                bf16_t val = (bf16_t)0.0f;
                if (c0 + c < C)
                    val = A[((ll)(s * P + p) * TL + 2 * kp + i2) * VA
                            + (s0 + c0 + c)];
                a_sm[p][kp][c][i2] = val;
            }
            __syncthreads();
            // --- corr: thread = (chalf, p, v); 4 c's per thread
            {
                int v = tid & 63;
                int p = (tid >> 6) & 3;
                int chalf = tid >> 8;
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                if (v0 + v < VB) {
                    bf16x2_t bp[KP];
                    const bf16_t* brow =
                        B + ((ll)(s * P + p) * TL) * VB + (v0 + v);
                    #pragma unroll
                    for (int kp = 0; kp < KP; ++kp) {
                        bf16x2_t t;
                        t[0] = *(const __bf16*)&brow[(ll)(2 * kp) * VB];
                        t[1] = *(const __bf16*)
                            &brow[(ll)(2 * kp + 1) * VB];
                        bp[kp] = t;
                    }
                    #pragma unroll
                    for (int kp = 0; kp < KP; ++kp) {
                        bf16x8 raw =
                            *(const bf16x8*)&a_sm[p][kp][chalf * 4][0];
                        #pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            short2_t s2 = {raw[2 * j], raw[2 * j + 1]};
                            acc[j] = __builtin_amdgcn_fdot2_f32_bf16(
                                __builtin_bit_cast(bf16x2_t, s2),
                                bp[kp], acc[j], false);
                        }
                    }
                }
                #pragma unroll
                for (int j = 0; j < 4; ++j)
                    corr_s[chalf * 4 + j][p][v] = acc[j];
            }
            __syncthreads();
            // --- normalize (thread = (c, v)) straight into z_smem
            {
                int c = wv;            // 8 waves = 8 c's
                int v = lane;
                float z[P];
                float mean = 0.f, sq = 0.f;
                #pragma unroll
                for (int p = 0; p < P; ++p) {
                    z[p] = fisher_z(corr_s[c][p][v]);
                    mean += z[p]; sq += z[p] * z[p];
                }
                mean /= (float)P;
                float var = sq / (float)P - mean * mean;
                float inv = (var <= 0.f) ? 0.f : rsqrtf(var);
                #pragma unroll
                for (int p = 0; p < P; ++p)
                    z_smem[c][s * P + p][v] =
                        (bf16_t)((z[p] - mean) * inv);
            }
            __syncthreads();
        }
        // --- Gram rank-64 update: wave wv owns voxel c0+wv.
        // z reads of this window finish before the next window's first
        // barrier, so no extra sync is needed here.
        {
            const int frow = lane & 15;
            #pragma unroll
            for (int ks = 0; ks < FG_VT / 32; ++ks) {
                const int fk = 8 * (lane >> 4) + 32 * ks;
                bf16x8 f[4];
                #pragma unroll
                for (int bnd = 0; bnd < 4; ++bnd)
                    f[bnd] = (bf16x8)(*(const bf16x8_u*)
                        &z_smem[wv][bnd * 16 + frow][fk]);
                int t = 0;
                #pragma unroll
                for (int i = 0; i < 4; ++i)
                    #pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j >= i)
                            G[t] =
                                __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                    f[i], f[j], G[t], 0, 0, 0), ++t;
            }
        }
        __syncthreads();
    }

    if (c0 + wv < C) {
        float* Gc = Gpart + ((vs * C) + c0 + wv) * (ll)(E * E);
        const int dcol = lane & 15;
        const int drow = (lane >> 4) * 4;
        int t = 0;
        #pragma unroll
        for (int i = 0; i < 4; ++i)
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < i) continue;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float val = G[t][r];
                    Gc[(ll)(i * 16 + drow + r) * E + j * 16 + dcol] =
                        val;
                    if (i != j)
                        Gc[(ll)(j * 16 + dcol) * E + i * 16 + drow + r]
                            = val;
                }
                ++t;
            }
    }
}

// ===========================================================================
// k_gram_bf16: G_c = Z_c Z_c^T per voxel with bf16 MFMA.
// Z: [C, E, V] bf16; G: [C, E, E] fp32.  E % 64 == 0 (host pads).
// Block = (c, band_i, band_j>=band_i); 4 waves own the 32x32 quadrants.
// ===========================================================================
#define GR_KT 128
#define GR_PAD 8
#define GR_ROW (GR_KT + GR_PAD)

// NP = 0: Z is pre-normalized; NP in {2,4}: Z holds RAW correlations
// and each staged tile gets Fisher-z + within-subject z-score applied
// in LDS before the MFMAs read it.  The normalize VALU work runs in
// this kernel's memory-latency shadow (PMC: 84 % WAIT_ANY) instead of
// the issue-bound corr kernel.  Subject groups (NP consecutive rows)
// never straddle the 64-row bands (E % NP == 0, 64 % NP == 0).
// DZ = dual-band staging needed (E > 64).  With E == 64 every block
// is its own diagonal band and zj is never read — eliding it halves
// the static LDS (34.8 -> 17.4 KB) and doubles how many corr blocks
// can co-reside with gram blocks inside the duo kernel.
template <int NP = 0, bool DZ = true>
__device__ __forceinline__ void gram_bf16_body(
    ll b,
    const bf16_t* __restrict__ Z, float* __restrict__ G,
    ll C, ll E, ll V, ll nsplit) {
    // nsplit > 1: V is cut into k-tile-aligned ranges, one partial G
    // per range (host sums) — keeps the chip full when C is small
    // (MALL-resident Z slabs want 32-voxel chunks; 32 blocks would
    // leave 7/8 of the CUs idle)
    const ll eb = E / 64;
    const ll ns = b % nsplit; b /= nsplit;
    const ll band_j = b % eb; b /= eb;
    const ll band_i = b % eb; b /= eb;
    const ll c = b;
    if (c >= C || band_j < band_i) return;
    const ll ktAll = (V + GR_KT - 1) / GR_KT;
    const ll ktPer = (ktAll + nsplit - 1) / nsplit;
    const ll kt0 = ns * ktPer;
    const ll kt1 = min(ktAll, kt0 + ktPer);
    if (kt0 >= kt1) {   // empty range: zero this partial
        for (ll i = threadIdx.x; i < E * E; i += 256)
            G[(ns * C + c) * E * E + i] = 0.0f;
        return;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int wr = (w >> 1) * 32;
    const int wc = (w & 1) * 32;

    __shared__ bf16_t zi[64][GR_ROW];
    __shared__ bf16_t zj[DZ ? 64 : 1][GR_ROW];
    const bool diag = !DZ || (band_i == band_j);
    const bf16_t* Zc = Z + c * E * V;
    const ll rows_i = band_i * 64;
    const ll rows_j = band_j * 64;

    f32x4 acc00 = (f32x4)0.f, acc01 = (f32x4)0.f;
    f32x4 acc10 = (f32x4)0.f, acc11 = (f32x4)0.f;

    // T14 issue-early/write-late staging: each thread holds the NEXT
    // K-tile (2x bf16x8 = 32 B) in registers while MFMAs consume the
    // CURRENT tile from LDS, so the HBM latency hides under compute
    // instead of draining at the barrier.
    //
    // NP == 0 (pre-normalized Z): thread owns one ROW's 32 columns.
    // NP > 0 (raw correlations): thread owns a [4 rows x 8 cols]
    // block — the rows cover whole subject groups, so Fisher-z + the
    // z-score run IN REGISTERS between the global load and the LDS
    // write: no extra barrier and no LDS round trip for the
    // normalize (the phase-after-staging form measured +1.4 ms).
    const int srow = (NP > 0) ? (tid >> 4) * 4 : (tid >> 2);
    const int scol = (NP > 0) ? (tid & 15) * 8 : (tid & 3) * 32;

    auto issue_loads = [&](const bf16_t* src, ll rows0, ll k0,
                           bf16x8 regs[4]) {
        #pragma unroll
        for (int h = 0; h < 4; ++h) {
            // NP==0: 4 chunks of row srow; NP>0: rows srow..srow+3,
            // one 8-col chunk each
            const int r = (NP > 0) ? h : 0;
            ll kk = k0 + scol + ((NP > 0) ? 0 : 8 * h);
            const bf16_t* s = src + (rows0 + srow + r) * V + kk;
            if (kk + 8 <= V && (((uintptr_t)s) & 3) == 0) {
                regs[h] = (bf16x8)(*(const bf16x8_u*)s);
            } else {
                bf16_t tmp[8];
                #pragma unroll
                for (int j = 0; j < 8; ++j)
                    tmp[j] = (kk + j < V) ? s[j] : (bf16_t)0.0f;
                regs[h] = *(const bf16x8*)tmp;
            }
        }
    };
    auto write_tile = [&](bf16_t dst[64][GR_ROW], bf16x8 regs[4]) {
        if (NP > 0) {
            // normalize the [4 x 8] register block column-wise over
            // each NP-row subject group, then store the 4 rows
            #pragma unroll
            for (int sub = 0; sub < 4 / (NP > 0 ? NP : 4); ++sub) {
                #pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float z[NP > 0 ? NP : 1];
                    float mean = 0.f, sq = 0.f;
                    #pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        __bf16 raw = __builtin_bit_cast(
                            __bf16, (short)regs[sub * NP + p][j]);
                        z[p] = fisher_z_unscaled((float)raw);
                        mean += z[p]; sq += z[p] * z[p];
                    }
                    mean /= (float)(NP > 0 ? NP : 1);
                    float var = sq / (float)(NP > 0 ? NP : 1)
                              - mean * mean;
                    float inv = (var <= 0.f) ? 0.f : rsqrtf(var);
                    #pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        bf16_t zb = (bf16_t)((z[p] - mean) * inv);
                        regs[sub * NP + p][j] = __builtin_bit_cast(
                            short, (__bf16)zb);
                    }
                }
            }
            #pragma unroll
            for (int r = 0; r < 4; ++r)
                *(bf16x8*)&dst[srow + r][scol] = regs[r];
            return;
        }
        #pragma unroll
        for (int h = 0; h < 4; ++h)
            *(bf16x8*)&dst[srow][scol + 8 * h] = regs[h];
    };

    bf16x8 ri[4], rj[4];
    issue_loads(Zc, rows_i, kt0 * GR_KT, ri);
    if (!diag) issue_loads(Zc, rows_j, kt0 * GR_KT, rj);

    for (ll kt = kt0; kt < kt1; ++kt) {
        __syncthreads();              // previous tile's reads complete
        write_tile(zi, ri);
        if (!diag) write_tile(zj, rj);
        if (kt + 1 < kt1) {           // issue next tile early
            issue_loads(Zc, rows_i, (kt + 1) * GR_KT, ri);
            if (!diag) issue_loads(Zc, rows_j, (kt + 1) * GR_KT, rj);
        }
        __syncthreads();              // tile visible
        const int frow = lane & 15;
        #pragma unroll
        for (int ks = 0; ks < GR_KT / 32; ++ks) {
            const int fk = 8 * (lane >> 4) + 32 * ks;
            bf16x8 fi0 = *(const bf16x8*)&zi[wr + frow][fk];
            bf16x8 fi1 = *(const bf16x8*)&zi[wr + 16 + frow][fk];
            const bf16_t (*zjs)[GR_ROW] = diag ? zi : zj;
            bf16x8 fj0 = *(const bf16x8*)&zjs[wc + frow][fk];
            bf16x8 fj1 = *(const bf16x8*)&zjs[wc + 16 + frow][fk];
            acc00 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fi0, fj0,
                                                            acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fi0, fj1,
                                                            acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fi1, fj0,
                                                            acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fi1, fj1,
                                                            acc11, 0, 0, 0);
        }
    }

    float* Gc = G + (ns * C + c) * E * E;
    const int dcol = lane & 15;
    const int drow = (lane >> 4) * 4;
    const f32x4* accs[4] = {&acc00, &acc01, &acc10, &acc11};
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
        int mi = q >> 1, ni = q & 1;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            ll gr = rows_i + wr + 16 * mi + drow + r;
            ll gc = rows_j + wc + 16 * ni + dcol;
            float val = (*accs[q])[r];
            Gc[gr * E + gc] = val;
            if (!diag || gr != gc) Gc[gc * E + gr] = val;
        }
    }
}

// DZ resolved at LAUNCH (host knows E): a runtime branch would leave
// BOTH bodies' static __shared__ arrays allocated in one kernel
// (52 KB instead of 17/35 — measured occupancy 3 vs 5)
template <int NP = 0, bool DZ = true>
__global__ __launch_bounds__(256) void k_gram_bf16(
    const bf16_t* __restrict__ Z, float* __restrict__ G,
    ll C, ll E, ll V, ll nsplit) {
    gram_bf16_body<NP, DZ>(blockIdx.x, Z, G, C, E, V, nsplit);
}

// ===========================================================================
// gsum_body: one block per selected voxel c — sums the nsplit
// partial Gram slabs of a FINISHED chunk into the final [E, E]
// matrix and applies the reference's magnitude shrink in the same
// pass.  Folding this into the duo grid removes the per-chunk torch
// reduce + shrink launches (~3.3 ms serial per whole-brain step) and
// hides the 143 MB partial re-read under the latency-bound corr/gram
// waves.
__device__ __forceinline__ void gsum_body(
    ll b, const float* __restrict__ Gp, float* __restrict__ Gout,
    ll Cs, ll EE, ll nsplit, int do_shrink) {
    const ll c = b;
    if (c >= Cs) return;
    const float* base = Gp + c * EE;
    const ll cstride = Cs * EE;
    float scale = 1.0f;
    if (do_shrink) {
        float lead = 0.0f;
        for (ll s = 0; s < nsplit; ++s)
            lead += base[s * cstride];
        lead = fmaxf(fabsf(lead), 1.0f);
        float digits = floorf(log10f(lead)) + 1.0f;
        if (digits > 2.0f)
            scale = powf(10.0f, 2.0f - digits);
    }
    for (ll el = threadIdx.x; el < EE; el += 256) {
        float acc = 0.0f;
        for (ll s = 0; s < nsplit; ++s)
            acc += base[s * cstride + el];
        Gout[c * EE + el] = acc * scale;
    }
}

// k_corr_gram_duo: ONE grid carrying BOTH the raw-correlation blocks of
// chunk i and the Gram(+normalize) blocks of chunk i-1, proportionally
// interleaved over blockIdx.  HIP streams do not co-schedule these two
// kernels (measured: exactly serial); a single grid forces CU-level
// co-residency, pairing the VALU-bound corr waves with the
// memory-latency-bound Gram waves.
// ===========================================================================
template <int TP, int TL, int NP, bool DZ = true, int CT = 128>
__global__ __launch_bounds__(256) void k_corr_gram_duo(
    const bf16_t* __restrict__ At, const bf16_t* __restrict__ B,
    bf16_t* __restrict__ zOut, ll E, ll VB, ll C, ll zstride,
    const bf16_t* __restrict__ Zprev, float* __restrict__ G,
    ll Cg, ll Eg, ll Vg, ll nsplit,
    const float* __restrict__ GpSum, float* __restrict__ GSumOut,
    ll Cs, ll nsplitSum, int do_shrink,
    ll nCorr, ll nGram, ll nSum) {
    ll b = blockIdx.x;
    const ll total = nCorr + nGram + nSum;
    // proportional interleave over THREE populations: first peel the
    // gsum quota (chunk i-2 partial reduction), then split the rest
    // between gram (chunk i-1) and corr (chunk i) blocks
    const ll s_before = (b * nSum) / total;
    const ll s_at = ((b + 1) * nSum) / total;
    if (s_at != s_before) {
        if (GSumOut != nullptr)
            gsum_body(s_before, GpSum, GSumOut, Cs, Eg * Eg,
                      nsplitSum, do_shrink);
        return;
    }
    b -= s_before;
    const ll rest = nCorr + nGram;
    const ll g_before = (b * nGram) / rest;
    const ll g_at = ((b + 1) * nGram) / rest;
    if (g_at != g_before) {
        if (G != nullptr)
            gram_bf16_body<NP, DZ>(g_before, Zprev, G, Cg, Eg, Vg,
                                   nsplit);
    } else {
        ll ci = b - g_before;        // corr block index
        if (ci < nCorr)
            dot3s_body<TP, TL, CT, bf16_t, true>(
                ci, At, B, zOut, E, VB, C, /*mode=*/0, zstride);
    }
}

// debug probe: elementwise to_fp8 over a float array (conversion
// semantics validation vs torch's e4m3fn — see tests/ops)
__global__ void k_fp8_cvt_probe(const float* __restrict__ x,
                                fp8_t* __restrict__ o, ll n) {
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = to_fp8(x[i]);
}

extern "C" void launch_fp8_cvt_probe(const float* x, void* o, ll n,
                                     hipStream_t stream) {
    hipLaunchKernelGGL(k_fp8_cvt_probe, dim3((n + 255) / 256), dim3(256),
                       0, stream, x, (fp8_t*)o, n);
}

// the header's software (bit-exact) conversion path, for A/B against
// the hardware cvt instruction the __hip_fp8_e4m3 ctor uses on gfx950
__global__ void k_fp8_cvt_probe_sw(const float* __restrict__ x,
                                   fp8_t* __restrict__ o, ll n) {
    ll i = (ll)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        o[i] = __hip_cvt_float_to_fp8(x[i], __HIP_SATFINITE, __HIP_E4M3);
}

extern "C" void launch_fp8_cvt_probe_sw(const float* x, void* o, ll n,
                                        hipStream_t stream) {
    hipLaunchKernelGGL(k_fp8_cvt_probe_sw, dim3((n + 255) / 256),
                       dim3(256), 0, stream, x, (fp8_t*)o, n);
}

// ===========================================================================
// k_gram_fp8: G_c = Z_c Z_c^T per voxel with fp8(e4m3) MFMA
// (v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulate).  Z: [C, E, V] fp8,
// V % 16 == 0 (host pads voxels); G: [C, E, E] fp32; E % 64 == 0.
// Same band/V-split decomposition and T14 issue-early staging as
// k_gram_bf16, but each staged tile carries 256 voxels in the same
// 16 KB — the Z re-read from HBM halves (profiles/NEXT.md item 1).
// ===========================================================================
#define G8_KT 256
#define G8_PAD 8
#define G8_ROW (G8_KT + G8_PAD)

__global__ __launch_bounds__(256) void k_gram_fp8(
    const fp8_t* __restrict__ Z, float* __restrict__ G,
    ll C, ll E, ll V, ll nsplit) {
    const ll eb = E / 64;
    ll b = blockIdx.x;
    const ll ns = b % nsplit; b /= nsplit;
    const ll band_j = b % eb; b /= eb;
    const ll band_i = b % eb; b /= eb;
    const ll c = b;
    if (c >= C || band_j < band_i) return;
    const ll ktAll = (V + G8_KT - 1) / G8_KT;
    const ll ktPer = (ktAll + nsplit - 1) / nsplit;
    const ll kt0 = ns * ktPer;
    const ll kt1 = min(ktAll, kt0 + ktPer);
    if (kt0 >= kt1) {
        for (ll i = threadIdx.x; i < E * E; i += 256)
            G[(ns * C + c) * E * E + i] = 0.0f;
        return;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int wr = (w >> 1) * 32;
    const int wc = (w & 1) * 32;

    __shared__ fp8_t zi[64][G8_ROW];
    __shared__ fp8_t zj[64][G8_ROW];
    const bool diag = (band_i == band_j);
    const fp8_t* Zc = Z + c * E * V;
    const ll rows_i = band_i * 64;
    const ll rows_j = band_j * 64;

    f32x4 acc00 = (f32x4)0.f, acc01 = (f32x4)0.f;
    f32x4 acc10 = (f32x4)0.f, acc11 = (f32x4)0.f;

    // 64 rows x 256 B per tile; 4 threads per row, 4x16 B each.
    // V % 16 == 0 keeps every global load dword4-aligned.
    const int srow = tid >> 2;
    const int scol = (tid & 3) * 64;

    auto issue_loads = [&](const fp8_t* src, ll rows0, ll k0,
                           uint32x4 regs[4]) {
        #pragma unroll
        for (int h = 0; h < 4; ++h) {
            ll kk = k0 + scol + 16 * h;
            const fp8_t* sp = src + (rows0 + srow) * V + kk;
            if (kk + 16 <= V) {
                regs[h] = *(const uint32x4*)sp;
            } else {
                regs[h] = (uint32x4)0u;   // V is 16-padded: whole
            }                             // vector in or out of range
        }
    };
    auto write_tile = [&](fp8_t dst[64][G8_ROW], uint32x4 regs[4]) {
        #pragma unroll
        for (int h = 0; h < 4; ++h)
            *(uint32x4*)&dst[srow][scol + 16 * h] = regs[h];
    };

    uint32x4 ri[4], rj[4];
    issue_loads(Zc, rows_i, kt0 * G8_KT, ri);
    if (!diag) issue_loads(Zc, rows_j, kt0 * G8_KT, rj);

    for (ll kt = kt0; kt < kt1; ++kt) {
        __syncthreads();
        write_tile(zi, ri);
        if (!diag) write_tile(zj, rj);
        if (kt + 1 < kt1) {
            issue_loads(Zc, rows_i, (kt + 1) * G8_KT, ri);
            if (!diag) issue_loads(Zc, rows_j, (kt + 1) * G8_KT, rj);
        }
        __syncthreads();
        const int frow = lane & 15;
        #pragma unroll
        for (int ks = 0; ks < G8_KT / 32; ++ks) {
            const int fk = 8 * (lane >> 4) + 32 * ks;
            long fi0 = *(const long*)&zi[wr + frow][fk];
            long fi1 = *(const long*)&zi[wr + 16 + frow][fk];
            const fp8_t (*zjs)[G8_ROW] = diag ? zi : zj;
            long fj0 = *(const long*)&zjs[wc + frow][fk];
            long fj1 = *(const long*)&zjs[wc + 16 + frow][fk];
            acc00 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                fi0, fj0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                fi0, fj1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                fi1, fj0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                fi1, fj1, acc11, 0, 0, 0);
        }
    }

    float* Gc = G + (ns * C + c) * E * E;
    const int dcol = lane & 15;
    const int drow = (lane >> 4) * 4;
    const f32x4* accs[4] = {&acc00, &acc01, &acc10, &acc11};
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
        int mi = q >> 1, ni = q & 1;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            ll gr = rows_i + wr + 16 * mi + drow + r;
            ll gc = rows_j + wc + 16 * ni + dcol;
            float val = (*accs[q])[r];
            Gc[gr * E + gc] = val;
            if (!diag || gr != gc) Gc[gc * E + gr] = val;
        }
    }
}

// ===========================================================================
// k_gram_f32: the same contraction from fp32 via exact-f32 MFMA
// v_mfma_f32_16x16x4_f32 (A: lane l -> A[l&15][l>>4]).
// ===========================================================================
#define GF_KT 32
#define GF_PAD 4
#define GF_ROW (GF_KT + GF_PAD)

__global__ __launch_bounds__(256) void k_gram_f32(
    const float* __restrict__ Zf, float* __restrict__ G,
    ll C, ll E, ll V) {
    const ll eb = E / 64;
    ll b = blockIdx.x;
    const ll band_j = b % eb; b /= eb;
    const ll band_i = b % eb; b /= eb;
    const ll c = b;
    if (c >= C || band_j < band_i) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int wr = (w >> 1) * 32;
    const int wc = (w & 1) * 32;

    __shared__ float zi[2][64][GF_ROW];
    __shared__ float zj[2][64][GF_ROW];
    const bool diag = (band_i == band_j);
    const float* Zc = Zf + c * E * V;
    const ll rows_i = band_i * 64;
    const ll rows_j = band_j * 64;

    f32x4 acc00 = (f32x4)0.f, acc01 = (f32x4)0.f;
    f32x4 acc10 = (f32x4)0.f, acc11 = (f32x4)0.f;

    auto load_tile = [&](float dst[64][GF_ROW], const float* src,
                         ll rows0, ll k0) {
        int row = tid >> 2;
        int col = (tid & 3) * 8;
        const float* s = src + (rows0 + row) * V + k0 + col;
        #pragma unroll
        for (int j = 0; j < 8; ++j)
            dst[row][col + j] = (k0 + col + j < V) ? s[j] : 0.0f;
    };

    const ll kTiles = (V + GF_KT - 1) / GF_KT;
    int cur = 0;
    load_tile(zi[0], Zc, rows_i, 0);
    if (!diag) load_tile(zj[0], Zc, rows_j, 0);
    __syncthreads();

    for (ll kt = 0; kt < kTiles; ++kt) {
        if (kt + 1 < kTiles) {
            load_tile(zi[cur ^ 1], Zc, rows_i, (kt + 1) * GF_KT);
            if (!diag) load_tile(zj[cur ^ 1], Zc, rows_j, (kt + 1) * GF_KT);
        }
        const int frow = lane & 15;
        const int fk0 = lane >> 4;
        #pragma unroll
        for (int step = 0; step < GF_KT / 4; ++step) {
            float ai0 = zi[cur][wr + frow][fk0 + 4 * step];
            float ai1 = zi[cur][wr + 16 + frow][fk0 + 4 * step];
            const float (*zjs)[GF_ROW] = diag ? zi[cur] : zj[cur];
            float aj0 = zjs[wc + frow][fk0 + 4 * step];
            float aj1 = zjs[wc + 16 + frow][fk0 + 4 * step];
            acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(ai0, aj0, acc00,
                                                         0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(ai0, aj1, acc01,
                                                         0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(ai1, aj0, acc10,
                                                         0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(ai1, aj1, acc11,
                                                         0, 0, 0);
        }
        __syncthreads();
        cur ^= 1;
    }

    float* Gc = G + c * E * E;
    const int dcol = lane & 15;
    const int drow = (lane >> 4) * 4;
    const f32x4* accs[4] = {&acc00, &acc01, &acc10, &acc11};
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
        int mi = q >> 1, ni = q & 1;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            ll gr = rows_i + wr + 16 * mi + drow + r;
            ll gc = rows_j + wc + 16 * ni + dcol;
            float val = (*accs[q])[r];
            Gc[gr * E + gc] = val;
            if (!diag || gr != gc) Gc[gc * E + gr] = val;
        }
    }
}

// ===========================================================================
// host-side launchers
// ===========================================================================

static inline ll ceil_div(ll a, ll b) { return (a + b - 1) / b; }

// The corr kernels' compile-time epoch lengths, written once: the host
// pads L up to the next entry (zero rows are inert for z-scored epochs).
constexpr int kSupportedL[] = {8, 12, 16, 20, 24, 28, 32, 36, 40};
// k_fused_corr_gram is instantiated for these only
constexpr int kFusedL[] = {8, 16, 24, 32, 40};

extern "C" ll fcma_supported_L(ll L) {
    for (int opt : kSupportedL)
        if (L <= opt) return opt;
    return -1;
}

template <int V> using int_c = std::integral_constant<int, V>;

// Runtime L -> compile-time TL: calls f(int_c<TL>{}) for the entry of
// Ls equal to L; false (and no call) when there is none.
template <auto& Ls, class F, size_t... I>
static bool dispatch_l(ll L, F&& f, std::index_sequence<I...>) {
    return ((L == Ls[I] && (f(int_c<Ls[I]>{}), true)) || ...);
}

template <auto& Ls, class F>
static bool dispatch_l(ll L, F&& f) {
    return dispatch_l<Ls>(L, f, std::make_index_sequence<std::size(Ls)>{});
}

template <int TP, class F>
static bool dispatch_pl_at(ll L, F& f) {
    return dispatch_l<kSupportedL>(L, [&](auto tl) { f(int_c<TP>{}, tl); });
}

// Runtime (P, L) -> compile-time (TP, TL): calls f(int_c<TP>{},
// int_c<TL>{}) for the first entry of Ps that is P, or that is 0 (the
// kernels' runtime-P instantiation, which takes every P), and for L in
// kSupportedL.  Returns false, with nothing called, when (P, L) has no
// instantiation — the launchers hand that to their caller.
template <int... Ps, class F>
static bool dispatch_pl(int P, ll L, F&& f) {
    bool hit = false;
    (void)(((Ps == 0 || P == Ps)
            && (hit = dispatch_pl_at<Ps>(L, f), true)) || ...);
    return hit;
}

template <int TP>
static void launch_normalize_t(float* corr, ll C, ll E, ll V, int P,
                               hipStream_t stream) {
    ll nSubj = E / P;
    ll grid = C * nSubj * ceil_div(V, 256);
    hipLaunchKernelGGL((k_normalize<TP>), dim3(grid), dim3(256), 0, stream,
                       corr, C, E, V, P);
}

extern "C" void launch_fcma_normalize(float* corr, ll C, ll E, ll V, int P,
                                      hipStream_t stream) {
    switch (P) {
        case 2:  launch_normalize_t<2>(corr, C, E, V, P, stream); break;
        case 4:  launch_normalize_t<4>(corr, C, E, V, P, stream); break;
        case 8:  launch_normalize_t<8>(corr, C, E, V, P, stream); break;
        case 16: launch_normalize_t<16>(corr, C, E, V, P, stream); break;
        case 32: launch_normalize_t<32>(corr, C, E, V, P, stream); break;
        default: launch_normalize_t<0>(corr, C, E, V, P, stream); break;
    }
}

// host mirror of the dot2 kernel's TCT constexpr
static ll dot2_ct(int P) {
    return (P == 2 || P == 4) ? 32 : CN_CT;
}

// dynamic LDS of k_corr_norm_dot2: bf16 a_tile + fp32 corr tile
extern "C" int fcma_corr_norm_smem(ll L, int P) {
    ll ct = dot2_ct(P);
    size_t smem = (size_t)P * L * ct * sizeof(bf16_t)
                + (size_t)ct * P * CN_VT * sizeof(float);
    return (int)smem;
}

// The dispatch rule of the corr(+normalize) stage, in one place:
//   mode 0 (bf16 Z), At given, P in {2,4} -> k_corr_norm_dot3s<TP,TL,128>
//     (12.9 ms/step no-cv vs 16.5 for dot2 — profiles/README.md)
//   everything else                        -> k_corr_norm_dot2<TP,TL>
template <int TP, int TL>
static void launch_corr_norm_t(const void* A, const void* B, void* zOut,
                               float* fOut, ll E, ll L, ll VA, ll VB,
                               ll s0, ll C, int P, int mode, ll zstride,
                               hipStream_t stream, const void* At) {
    ll nSubj = E / P;
    if constexpr (TP == 2 || TP == 4) {
        if (mode == 0 && At != nullptr) {
            ll grid3 = ceil_div(C, 128) * nSubj * ceil_div(VB, C3_VT);
            hipLaunchKernelGGL((k_corr_norm_dot3s<TP, TL, 128>),
                               dim3(grid3), dim3(256), 0, stream,
                               (const bf16_t*)At, (const bf16_t*)B,
                               (bf16_t*)zOut, E, VB, C, mode, zstride);
            return;
        }
    }
    size_t smem = (size_t)fcma_corr_norm_smem(L, P);
    ll gridd = ceil_div(C, dot2_ct(P)) * nSubj * ceil_div(VB, CN_VT);
    if (smem > 64 * 1024) {
        // gfx950 has 160 KB LDS but dynamic allocations above the
        // 64 KB default need the explicit opt-in, once per kernel
        static bool raised = false;
        if (!raised) {
            (void)hipFuncSetAttribute(
                reinterpret_cast<const void*>(
                    &k_corr_norm_dot2<TP, TL>),
                hipFuncAttributeMaxDynamicSharedMemorySize,
                160 * 1024);
            raised = true;
        }
    }
    hipLaunchKernelGGL((k_corr_norm_dot2<TP, TL>), dim3(gridd),
                       dim3(256), smem, stream, (const bf16_t*)A,
                       (const bf16_t*)B, (bf16_t*)zOut, fOut, E, L,
                       VA, VB, s0, C, P, mode, zstride);
}

// The four (P, L)-templated launchers return 1, or 0 when (P, L) has no
// instantiation and nothing was launched.
extern "C" int launch_fcma_corr_norm(const void* A, const void* B,
                                     void* zOut, float* fOut, ll E, ll L,
                                     ll VA, ll VB, ll s0, ll C, int P,
                                     int mode, ll zstride,
                                     hipStream_t stream, const void* At) {
    return dispatch_pl<2, 4, 8, 16, 0>(P, L, [&](auto tp, auto tl) {
        launch_corr_norm_t<decltype(tp)::value, decltype(tl)::value>(
            A, B, zOut, fOut, E, L, VA, VB, s0, C, P, mode, zstride,
            stream, At);
    });
}

// raw-r variant: dot3s with the normalize deferred (bf16 Z only)
extern "C" int launch_fcma_corr_raw(const void* At, const void* B,
                                    void* zOut, ll E, ll L, ll VB,
                                    ll C, ll zstride, int P,
                                    hipStream_t stream) {
    ll nSubj = E / P;
    ll grid3 = ceil_div(C, 128) * nSubj * ceil_div(VB, C3_VT);
    return dispatch_pl<2, 4>(P, L, [&](auto tp, auto tl) {
        constexpr int TP = decltype(tp)::value, TL = decltype(tl)::value;
        hipLaunchKernelGGL((k_corr_norm_dot3s<TP, TL, 128, bf16_t, true>),
                           dim3(grid3), dim3(256), 0, stream,
                           (const bf16_t*)At, (const bf16_t*)B,
                           (bf16_t*)zOut, E, VB, C, /*mode=*/0, zstride);
    });
}

// fp8-output corr+normalize: the dot3s kernel with an e4m3 Z store.
// P in {2, 4}, even L (the production dot3s envelope); At required.
extern "C" int fcma_corr_norm_z8_supported(ll E, int P, ll L) {
    return (P == 2 || P == 4) && (L % 2) == 0 && (E % P) == 0;
}

extern "C" int launch_fcma_corr_norm_z8(const void* At, const void* B,
                                        void* zOut, ll E, ll L, ll VB,
                                        ll C, ll zstride,
                                        int P, hipStream_t stream) {
    ll nSubj = E / P;
    ll grid3 = ceil_div(C, 128) * nSubj * ceil_div(VB, C3_VT);
    return dispatch_pl<2, 4>(P, L, [&](auto tp, auto tl) {
        constexpr int TP = decltype(tp)::value, TL = decltype(tl)::value;
        hipLaunchKernelGGL((k_corr_norm_dot3s<TP, TL, 128, fp8_t>),
                           dim3(grid3), dim3(256), 0, stream,
                           (const bf16_t*)At, (const bf16_t*)B,
                           (fp8_t*)zOut, E, VB, C, /*mode=*/0, zstride);
    });
}

extern "C" ll fcma_duo_gram_blocks(ll Cg, ll Eg, ll nsplit) {
    ll eb = Eg / 64;
    return Cg * eb * eb * nsplit;
}

// duo grid: 128-voxel corr tiles (a 64-voxel tile measured 2 % slower —
// profiles/README.md), DZ by whether the Gram has more than one band
extern "C" int launch_fcma_corr_gram_duo(
    const void* At, const void* B, void* zOut, ll E, ll L, ll VB, ll C,
    ll zstride, int P,
    const void* Zprev, float* G, ll Cg, ll Eg, ll Vg, ll nsplit,
    const float* GpSum, float* GSumOut, ll Cs, ll nsplitSum,
    int do_shrink, hipStream_t stream) {
    ll nSubj = E / P;
    ll nCorr = ceil_div(C, 128) * nSubj * ceil_div(VB, C3_VT);
    ll nGram = (G != nullptr) ? fcma_duo_gram_blocks(Cg, Eg, nsplit)
                              : 0;
    ll nSum = (GSumOut != nullptr) ? Cs : 0;
    ll grid = nCorr + nGram + nSum;
    const bool dz = (Eg != 64);
    return dispatch_pl<2, 4>(P, L, [&](auto tp, auto tl) {
        constexpr int TP = decltype(tp)::value, TL = decltype(tl)::value;
        auto launch = [&](auto dzc) {
            constexpr bool DZ = decltype(dzc)::value;
            hipLaunchKernelGGL((k_corr_gram_duo<TP, TL, TP, DZ, 128>),
                               dim3(grid), dim3(256), 0, stream,
                               (const bf16_t*)At, (const bf16_t*)B,
                               (bf16_t*)zOut, E, VB, C, zstride,
                               (const bf16_t*)Zprev, G, Cg, Eg, Vg,
                               nsplit, GpSum, GSumOut, Cs, nsplitSum,
                               do_shrink, nCorr, nGram, nSum);
        };
        if (dz) launch(std::true_type{});
        else    launch(std::false_type{});
    });
}

// single-kernel chunk path: E = 64, P = 4 and an instantiated L
extern "C" int fcma_fused_gram_supported(ll E, int P, ll L) {
    return E == 64 && P == 4 && dispatch_l<kFusedL>(L, [](auto) {});
}

extern "C" int launch_fcma_fused_corr_gram(
    const void* A, const void* B, float* Gpart, ll L, ll VA, ll VB,
    ll s0, ll C, int nsplit, hipStream_t stream) {
    ll grid = ((C + FG_CB - 1) / FG_CB) * nsplit;
    return dispatch_l<kFusedL>(L, [&](auto tl) {
        hipLaunchKernelGGL((k_fused_corr_gram<decltype(tl)::value>),
                           dim3(grid), dim3(512), 0, stream,
                           (const bf16_t*)A, (const bf16_t*)B, Gpart, VA,
                           VB, s0, C, nsplit);
    });
}

extern "C" void launch_fcma_gram_bf16(const void* Z, float* G, ll C, ll E,
                                      ll V, ll nsplit,
                                      hipStream_t stream) {
    ll eb = E / 64;
    ll grid = C * eb * eb * nsplit;
    if (E == 64)
        hipLaunchKernelGGL((k_gram_bf16<0, false>), dim3(grid),
                           dim3(256), 0, stream, (const bf16_t*)Z, G, C,
                           E, V, nsplit);
    else
        hipLaunchKernelGGL((k_gram_bf16<0, true>), dim3(grid),
                           dim3(256), 0, stream, (const bf16_t*)Z, G, C,
                           E, V, nsplit);
}

extern "C" void launch_fcma_gram_bf16_norm(const void* Z, float* G,
                                           ll C, ll E, ll V, ll nsplit,
                                           int P, hipStream_t stream) {
    ll eb = E / 64;
    ll grid = C * eb * eb * nsplit;
    #define GRAM_NORM_CASE(NP, DZ)                                       \
        hipLaunchKernelGGL((k_gram_bf16<NP, DZ>), dim3(grid),            \
                           dim3(256), 0, stream, (const bf16_t*)Z, G,    \
                           C, E, V, nsplit)
    if (E == 64) {
        if (P == 4) GRAM_NORM_CASE(4, false);
        else        GRAM_NORM_CASE(2, false);
    } else {
        if (P == 4) GRAM_NORM_CASE(4, true);
        else        GRAM_NORM_CASE(2, true);
    }
    #undef GRAM_NORM_CASE
}


extern "C" void launch_fcma_gram_fp8(const void* Z, float* G, ll C, ll E,
                                     ll V, ll nsplit,
                                     hipStream_t stream) {
    ll eb = E / 64;
    ll grid = C * eb * eb * nsplit;
    hipLaunchKernelGGL(k_gram_fp8, dim3(grid), dim3(256), 0, stream,
                       (const fp8_t*)Z, G, C, E, V, nsplit);
}


extern "C" void launch_fcma_gram_f32(const float* Z, float* G, ll C, ll E,
                                     ll V, hipStream_t stream) {
    ll eb = E / 64;
    ll grid = C * eb * eb;
    hipLaunchKernelGGL(k_gram_f32, dim3(grid), dim3(256), 0, stream,
                       Z, G, C, E, V);
}

// stand-alone gsum: fixed-order reduction (+ shrink) of [nsplit, C, E, E]
// partials for callers that have no duo grid to ride
__global__ __launch_bounds__(256) void k_gsum(
    const float* __restrict__ Gp, float* __restrict__ Gout, ll Cs, ll EE,
    ll nsplit, int do_shrink) {
    gsum_body(blockIdx.x, Gp, Gout, Cs, EE, nsplit, do_shrink);
}

extern "C" void launch_fcma_gsum(const float* Gp, float* Gout, ll Cs,
                                 ll EE, ll nsplit, int do_shrink,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(k_gsum, dim3(Cs), dim3(256), 0, stream, Gp, Gout,
                       Cs, EE, nsplit, do_shrink);
}
