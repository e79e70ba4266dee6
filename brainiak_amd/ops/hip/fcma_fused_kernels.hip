// k_corr_gram_fused: correlation (MFMA) + Fisher-z / within-subject
// z-score (registers) + per-voxel Gram (MFMA) in ONE kernel for gfx950.
// The [count, 64, V] intermediate never leaves the CU: each window of
// normalized z lives in LDS only.
//
// Operands are the time-contiguous cached layout T[64][V][LP] bf16
// (epoch rows >= E and time steps >= L are zero), LP in {16, 32, 64}.
// They must be finite: stack_epochs zero-pads and callers z-score with
// a clamped std.  The clamp test below takes a NaN variance for the
// mark of a 1 +- r <= 0; a NaN that came in with the operands would send
// its task through the clamped normalize as well.
// Columns at or past VB (VB % 16 == 0) are read as zeros: the column
// loads go through buffer descriptors whose range ends with the epoch
// row, so a dead 16-column sub-tile has r = 0, z = 0, var = 0 and stores
// z = 0 by the var <= 0 select, with no test of its own.
//
// Work split: a 512-thread workgroup (FS_NW = 8 waves, one per CU)
// owns FS_CB = 16 selected voxels and sweeps a contiguous range of
// FS_VT = 32-column windows of data2.
//
//  phase 1  wave w takes subjects s = w, w+8, ... and both 16-column
//           sub-tiles.  Per epoch one MFMA (two k-steps for LP = 64) with
//             A (M = column v)  : lane l -> T2[e][v0 + l%16][k-seg(l)]
//             B (N = voxel  c)  : lane l -> T1[e][c0 + l%16][k-seg(l)]
//           so the accumulator holds c = lane&15 on the lane and the
//           four consecutive columns v = 4*(lane>>4) + reg in its regs.
//           The P accumulators of a subject sit in the same lane.
//           The wave's B fragments (its subjects' selected-voxel rows)
//           are the same for every window: they are loaded once and
//           stay in registers for the sweep.  A task is one (subject,
//           sub-tile) pair; in the AHEAD order (below, LP <= 32) task
//           t+1's MFMAs are issued before task t's normalize.
//  phase 2  per element: r -> bf16 -> fp32, Fisher z, biased mean/var
//           over P, (z - mean) * rsq(var) (var <= 0 -> 0; var is never
//           denormal, so the raw v_rsq_f32 equals rsqrtf bit for bit),
//           bf16; the 4 columns pack into one 8-byte LDS store into
//           z[c][e][v].  The clamp of the Fisher z (max(1 +- r, 1e-4))
//           only matters where the bf16 r reaches |r| >= 1, about one
//           window of a sweep.  Nobody looks for such an r ahead: every
//           task runs the unclamped normalize, and always and only
//           where some 1 +- r <= 0 the log is -inf or NaN, the sum of
//           squares +inf and var = fma(sq, 1/P, -mean^2) a NaN.  Two
//           v_cmp_u_f32 per task (the lane's four variances, pairwise)
//           find that; the wave then normalizes the same correlations
//           again, clamped, before it stores.  The FORCE instances
//           (force_clamp) run the clamped normalize for every task and
//           test nothing.  Both give the same bits.  The TABLE
//           instances (LP <= 32, the default there) read the Fisher z
//           of the unclamped normalize from an LDS table of the bf16
//           magnitudes instead of computing four logs per pair
//           (fisher_z_table below); an |r| >= 1 reads a NaN entry, so
//           the NaN variance and the clamped redo stay as they are.
//  phase 3  wave w owns voxels 2w, 2w+1: four 16-row bands as bf16x8
//           fragments, the 10 upper-triangle 16x16x32 MFMAs per voxel;
//           accumulators (40 fp32 / voxel / lane) persist across the
//           sweep and the lower triangle is mirrored at the store.
//
// The z image is double-buffered, so there is ONE barrier per window:
// a wave that leaves the Gram of window w early starts the correlation
// and normalize of window w+1 while its neighbours still issue MFMAs.
// (Four waves x four voxels at two blocks per CU needs 160 accumulator
// registers per lane and spills; eight waves x two voxels does not.)
// LDS invariant: a wave has issued and waited for every Gram read of
// image w before it arrives at the barrier that ends window w+1,
// because window w+2 overwrites that image.  Here the reads sit right
// behind the barrier of window w, ahead of every store of window w+1.
//
// LDS image: voxel c at c * stride, row (c, e) 64 B = four 16-B chunks,
// chunk k in slot k ^ fs_img_swz(e).  The address functions, and what
// the banking of gfx950 asks of them, are in fcma_fused_image.h: a
// phase-2 ds_write_b64 is served in four contiguous 16-lane groups on
// banks (a/4) mod 32 (one group = the 16 voxels: the stride of
// 4096 + 16 B leaves it 2-way, the floor for this store), a Gram
// ds_read_b128 in four NON-contiguous 16-lane groups on banks
// (a/4) mod 64 (the swizzle 0, 3, 2, 1 of (e>>2)&3 makes each
// conflict-free).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "fcma_common.h"
#include "fcma_fused_image.h"

#define FS_CB 16
#define FS_VT 32
#define FS_E 64
#define FS_NW 8                                // waves per workgroup
#define FS_VPW (FS_CB / FS_NW)                 // Gram voxels per wave
// the z image's strides and offsets: fcma_fused_image.h
static_assert(FS_CB == FS_IMG_CB && FS_E == FS_IMG_E && FS_NW == FS_IMG_NW
              && FS_VT * 2 == FS_IMG_ROWB, "fcma_fused_image.h");

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 nbf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 nbf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 nbf16x8 __attribute__((ext_vector_type(8)));

// one lane's k-segment of a [.., LP] row: 4 bf16 for the 16x16x16
// form (LP == 16), 8 bf16 per 16x16x32 k-step otherwise
template <int LP> struct FragT { bf16x8 v; };
template <> struct FragT<16> { bf16x4 v; };

template <int LP>
__device__ __forceinline__ FragT<LP> load_frag(const bf16_t* row, int q,
                                               int ks) {
    FragT<LP> f;
    if constexpr (LP == 16)
        f.v = *(const bf16x4*)(row + 4 * q);
    else
        f.v = *(const bf16x8*)(row + 32 * ks + 8 * q);
    return f;
}

// the same k-segment through a buffer descriptor: voff is the lane's
// byte offset from the descriptor's base, bytes at or past num_records
// read as zero
template <int LP>
__device__ __forceinline__ FragT<LP> load_frag_buf(
    __amdgpu_buffer_rsrc_t rs, unsigned voff) {
    FragT<LP> f;
    if constexpr (LP == 16)
        f.v = __builtin_bit_cast(
            bf16x4, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 0, 0));
    else
        f.v = __builtin_bit_cast(
            bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
    return f;
}

template <int LP>
__device__ __forceinline__ f32x4 corr_mfma(const FragT<LP>& a,
                                           const FragT<LP>& b, f32x4 acc) {
    if constexpr (LP == 16) {
        // v_mfma_f32_16x16x16_bf16: lane l, j in 0..3 ->
        // A[l%16][4*(l>>4)+j], B[4*(l>>4)+j][l%16]
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.v, b.v, acc,
                                                         0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(nbf16x8, a.v),
            __builtin_bit_cast(nbf16x8, b.v), acc, 0, 0, 0);
    }
}

// Fisher z + within-subject z-score of one task: the P x 4 bf16-rounded
// correlations of one lane (four columns x the P epochs of a subject)
// -> P packed bf16x4.  CLAMP = true is fisher_z_unscaled_bf16r, CLAMP =
// false drops its two max(): for |r| < 1 on the bf16 grid 1 +- r is at
// least 2^-8, so the clamp is the identity and both forms give the
// same bits.  The columns go as the two pairs that came out of one
// bf16x2 convert, so everything but the logs is a packed f32 operation.
//
// Contraction is off and every fused multiply-add is spelled out: which
// product of a sum the compiler fuses changes the last bit, and it
// chose differently from one instantiation (and one loop copy) to the
// next.  The forms below are the ones all six instantiations had when
// the kernel was first measured and tested:
//   sq   = fma(z[P-1], z[P-1], ... fma(z0, z0, z1 * z1))
//   var  = fma(sq, 1/P, -(mean * mean)),  mean = sum * (1/P)
//   out  = fma(-sum, 1/P, z) * inv        (= (z - mean) * inv exactly)
// sum starts from z[0], not 0 + z[0]: a z from the logs is never -0
// (log2(1) is +0 and x - x is +0), so the add changed nothing.  (A z
// from the table can be -0; fisher_z_table says why no Gram sees it.)
//
// Returns the wave's lanes in which the unclamped form met a 1 +- r <= 0
// (CLAMP = false; always 0 for CLAMP = true).  There, and only there,
// some z is +-inf or NaN, so sq is +inf or NaN and var is NaN; for
// |r| < 1 everything is finite.  v_cmp_u_f32 takes two operands, so the
// four variances of a lane cost two compares, OR-ed on the scalar unit.
// z of one column pair: log2(1 + r) - log2(1 - r), the Fisher z up to
// the factor the z-score cancels
template <bool CLAMP>
__device__ __forceinline__ f32x2 fisher_z_log(f32x2 r2) {
    #pragma clang fp contract(off)
    f32x2 num = 1.0f + r2;
    f32x2 den = 1.0f - r2;
    if constexpr (CLAMP) {
        num[0] = __builtin_fmaxf(num[0], 1e-4f);
        num[1] = __builtin_fmaxf(num[1], 1e-4f);
        den[0] = __builtin_fmaxf(den[0], 1e-4f);
        den[1] = __builtin_fmaxf(den[1], 1e-4f);
    }
    const f32x2 ln = {__builtin_amdgcn_logf(num[0]),
                      __builtin_amdgcn_logf(num[1])};
    const f32x2 ld = {__builtin_amdgcn_logf(den[0]),
                      __builtin_amdgcn_logf(den[1])};
    return ln - ld;
}

// within-subject z-score of one column pair (half h of the lane's four
// columns) from its P Fisher z; CHECK adds the NaN-variance test
template <int P, bool CHECK>
__device__ __forceinline__ unsigned long long normalize_half(
    const f32x2 (&z)[P], int h, nbf16x4 (&zo)[P]) {
    #pragma clang fp contract(off)
    const f32x2 rP = (f32x2)(1.0f / (float)P);
    unsigned long long missed = 0;
    f32x2 sum = z[0];
    f32x2 sq = __builtin_elementwise_fma(z[0], z[0], z[1] * z[1]);
    sum += z[1];
    #pragma unroll
    for (int p = 2; p < P; ++p) {
        sum += z[p];
        sq = __builtin_elementwise_fma(z[p], z[p], sq);
    }
    const f32x2 mean = sum * rP;
    const f32x2 var = __builtin_elementwise_fma(sq, rP, -(mean * mean));
    if constexpr (CHECK)
        missed = __builtin_amdgcn_ballot_w64(
            __builtin_isunordered(var[0], var[1]));
    f32x2 inv;
    #pragma unroll
    for (int j = 0; j < 2; ++j)
        inv[j] = (var[j] <= 0.f) ? 0.f : __builtin_amdgcn_rsqf(var[j]);
    #pragma unroll
    for (int p = 0; p < P; ++p) {
        const f32x2 o = __builtin_elementwise_fma(-sum, rP, z[p]) * inv;
        zo[p][2 * h] = (__bf16)o[0];
        zo[p][2 * h + 1] = (__bf16)o[1];
    }
    return missed;
}

template <int P, bool CLAMP>
__device__ __forceinline__ unsigned long long normalize_task(
    const f32x4 (&rq)[P], nbf16x4 (&zo)[P]) {
    unsigned long long missed = 0;
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x2 z[P];
        #pragma unroll
        for (int p = 0; p < P; ++p) {
            const f32x2 r2 = {rq[p][2 * h], rq[p][2 * h + 1]};
            z[p] = fisher_z_log<CLAMP>(r2);
        }
        missed |= normalize_half<P, !CLAMP>(z, h, zo);
    }
    return missed;
}

// The Fisher z from a table.  Its argument has just been rounded to
// bf16, so z is a function of a 16-bit pattern.  It is exactly odd
// (ld - ln == -(ln - ld)), exactly +0 for |r| <= 2^-25 = 0x3300 (both
// 1 + r and 1 - r round to 1), and needs the clamp exactly for |r| >= 1
// = 0x3F80.  What is left are the magnitudes 0x3301 .. 0x3F7F:
//   entry 0            +0
//   entry i            fisher_z_log<false> of the magnitude 0x3300 + i
//   entry FS_TAB_LAST  a quiet NaN, for |r| >= 1, infinities and NaNs
// Every workgroup builds the table in LDS at kernel start with the very
// function the log path runs, so it holds that path's bits by
// construction.  The table lies at the start of the kernel's one LDS
// array: the index scaled to bytes is the ds_read address.
#define FS_TAB_LO 0x3300                       // 2^-25
#define FS_TAB_LAST (0x3F80 - FS_TAB_LO)       // 3200
#define FS_TAB_BYTES ((FS_TAB_LAST + 1) * 4 + 12)   // 16-byte multiple

__device__ __forceinline__ void fisher_table_build(float* tab, int tid,
                                                   int nthreads) {
    for (int i = tid; i <= FS_TAB_LAST; i += nthreads) {
        const float r = __builtin_bit_cast(
            float, (unsigned)(FS_TAB_LO + i) << 16);
        float z = fisher_z_log<false>((f32x2){r, r})[0];
        if (i == 0) z = 0.f;
        if (i == FS_TAB_LAST) z = __builtin_nanf("");
        tab[i] = z;
    }
}

// Byte offsets into the table of the two correlations a, b:
//   4 * min(sat_sub(|bf16(r)| as bits, FS_TAB_LO), FS_TAB_LAST)
// on the packed pair that comes out of the convert.  The sign bit goes
// with a packed shift by one, which leaves twice the magnitude, so the
// subtraction and the minimum run on doubled values; the second factor
// of two comes with the split into two addresses: v_mad_u32_u16 takes
// the low half times two, a shift by 15 the high half (twice the index
// is below 2^15, so nothing of the low half gets into it).  Eight
// instructions per pair with the two v_bfi_b32 of the sign.
// The compiler has no pattern for that multiply-add (it emits a mask
// and a shift, and that build measured 2.0 ms per pass slower), hence
// the asm; its source is the v_pk_min_u16 above.  The convert would
// take |x| source modifiers as well, but only through inline asm, and
// the compiler keeps no MFMA-to-VALU distance for a register that
// inline asm reads: the phased instances, whose correlations come
// straight out of the MFMAs, read stale registers that way and fail the
// bit tests.  No inline asm may read a correlation.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void fisher_table_offsets(float a, float b,
                                                     unsigned& lo,
                                                     unsigned& hi) {
    const f32x2 r2 = {a, b};
    const unsigned u = __builtin_bit_cast(
        unsigned, __builtin_convertvector(r2, nbf16x2));
    u16x2 i = __builtin_bit_cast(u16x2, u) << (u16x2)(unsigned short)1;
    i = __builtin_elementwise_sub_sat(
        i, (u16x2)(unsigned short)(2 * FS_TAB_LO));
    i = __builtin_elementwise_min(i,
                                  (u16x2)(unsigned short)(2 * FS_TAB_LAST));
    const unsigned x = __builtin_bit_cast(unsigned, i);
    // x must stay the result of a VALU instruction the compiler sees
    // (here the v_pk_min_u16), never an MFMA result: asm operands get no
    // MFMA wait states
    asm("v_mad_u32_u16 %0, %1, 2, 0" : "=v"(lo) : "v"(x));
    hi = x >> 15;
}

// z of one column pair of unrounded correlations.  The magnitude comes
// from the table, the sign from r itself (bf16 rounding keeps it).  A
// negative r with |r| <= 2^-25 therefore gives -0 where the log path
// gives +0 (log2(1) - log2(1)).  That zero stays: it can flip the sign
// of a zero in the z image and nothing else.  In the z-score a -0 adds
// like +0 to anything non-zero, var = fma(sq, 1/P, -(mean * mean)) is
// +0 + -0 = +0 either way, and the output is a zero of either sign.  In
// the Gram every product with it is a zero, the accumulators start at
// +0, and +0 plus a zero of either sign is +0 while anything else plus a
// zero is itself: no Gram bit depends on the sign.
__device__ __forceinline__ f32x2 fisher_z_table(f32x2 r2,
                                                const unsigned char* tab) {
    unsigned lo, hi;
    fisher_table_offsets(r2[0], r2[1], lo, hi);
    const float m0 = *(const float*)(tab + lo);
    const float m1 = *(const float*)(tab + hi);
    return (f32x2){__builtin_copysignf(m0, r2[0]),
                   __builtin_copysignf(m1, r2[1])};
}

// normalize_task<P, false> with the z from the table.  A task that holds
// an |r| >= 1 (or a non-finite r) reads the NaN entry, its variance is
// NaN, and the lanes come back as with the unclamped logs.
template <int P>
__device__ __forceinline__ unsigned long long normalize_task_table(
    const f32x4 (&r)[P], const unsigned char* tab, nbf16x4 (&zo)[P]) {
    unsigned long long missed = 0;
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x2 z[P];
        #pragma unroll
        for (int p = 0; p < P; ++p) {
            const f32x2 r2 = {r[p][2 * h], r[p][2 * h + 1]};
            z[p] = fisher_z_table(r2, tab);
        }
        missed |= normalize_half<P, true>(z, h, zo);
    }
    return missed;
}

// launch_fcma_corr_gram_fused's schedule argument (ext.cpp maps the
// strings "auto" / "ahead" / "phased" to these)
#define FS_SCHED_AUTO 0
#define FS_SCHED_AHEAD 1
#define FS_SCHED_PHASED 2

// AHEAD: the correlation MFMAs of task t+1 are issued before the
// normalize of task t, from column fragments loaded a whole task
// earlier (the column prefetch runs two tasks deep).  The MFMAs then
// never wait on their loads and their results are long there when the
// bf16 converts want them.  One-k-step instances only (LP <= 32): the
// second k-step of LP = 64 would need a third set of column fragments.
// AHEAD = false is the order the kernel was first shipped with (load one
// task ahead, MFMA at the head of its own task).  Both give the same
// bits: the same MFMAs on the same operands.
static constexpr bool fs_has_ahead(int LP) { return LP <= 32; }

// launch_fcma_corr_gram_fused's fisher argument ("auto" / "table" /
// "log").  TABLE: the unclamped normalize takes the Fisher z from the
// LDS table above; the redo of a task with a miss is the clamped log
// normalize as before.  One-k-step instances only: the LP = 64 instances
// stand at 255 VGPRs and keep the logs.  The FORCE instances keep them
// too and are the yardstick inside the build.
#define FS_FISHER_AUTO 0
#define FS_FISHER_TABLE 1
#define FS_FISHER_LOG 2
static constexpr bool fs_has_table(int LP) { return LP <= 32; }

template <int TP, int LP, bool AHEAD, bool FORCE, bool TABLE>
__global__ __launch_bounds__(64 * FS_NW) void k_corr_gram_fused(
    const bf16_t* __restrict__ T1, const bf16_t* __restrict__ T2,
    float* __restrict__ Gout, ll VA, ll VB, ll s0, ll C, int nsplit,
    int do_shrink) {
    constexpr int P = TP;
    constexpr int NSUBJ = FS_E / P;
    constexpr int SPW = NSUBJ / FS_NW;           // subjects per wave
    constexpr int KS = (LP + 31) / 32;         // MFMA k-steps
    constexpr int NT = 2 * SPW;                // tasks per window
    static_assert(!AHEAD || KS == 1, "AHEAD needs a one-k-step instance");
    static_assert(!TABLE || (KS == 1 && !FORCE),
                  "TABLE needs a one-k-step instance that finds its clamp");

    const ll vs = blockIdx.x % nsplit;
    const ll ct = blockIdx.x / nsplit;
    const ll c0 = ct * FS_CB;
    if (c0 >= C) return;
    const ll wAll = (VB + FS_VT - 1) / FS_VT;
    const ll wPer = (wAll + nsplit - 1) / nsplit;
    const ll w0 = vs * wPer;
    const ll w1 = min(wAll, w0 + wPer);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // wave index in an SGPR: everything derived from it (subject, epoch
    // row bases, LDS rows) then stays on the scalar unit
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15;
    const int q = lane >> 4;

    // one array, so that the table (TABLE only) starts at LDS address 0
    // and the two z images follow it
    constexpr unsigned TABB = TABLE ? FS_TAB_BYTES : 0;
    __shared__ __attribute__((aligned(16)))
        unsigned char lds[TABB + 2 * fs_img_bytes()];
    if constexpr (TABLE) {
        fisher_table_build((float*)lds, tid, 64 * FS_NW);
        __syncthreads();
    }

    // selected voxel of this lane (clamped: tail lanes recompute the
    // last voxel and are never stored)
    const ll csel = s0 + min(c0 + (ll)l16, C - 1);

    // wave-uniform row base + per-lane 32-bit element offset
    const unsigned sel_off = (unsigned)(csel * LP);
    auto sel_row = [&](int e) {
        return T1 + (ll)e * VA * LP + sel_off;
    };

    f32x4 G[FS_VPW][10];
    #pragma unroll
    for (int i = 0; i < FS_VPW; ++i)
        #pragma unroll
        for (int t = 0; t < 10; ++t) G[i][t] = (f32x4)0.f;

    // task (si, st): subject wv + FS_NW*si, 16-column sub-tile st.
    // Column fragments come through a buffer descriptor per epoch row and
    // sub-tile: base = the sub-tile's first column in that row, range =
    // what is left of the row (nothing at or past VB; VB % 16 == 0, so
    // whole sub-tiles).  Base and range are scalar (kernel arguments,
    // blockIdx, the wave index), so the range check sees the lane offset
    // alone, whatever it does with soffset; the lane keeps one constant
    // byte offset for the sweep.  A dead sub-tile reads zeros: r = 0,
    // z = 0, var = 0 and the var <= 0 select stores z = 0.
    const unsigned col_voff = (unsigned)(l16 * LP * 2)
        + (LP == 16 ? 8u * q : 16u * q);
    auto load_cols = [&](ll v0, int si, int st, int ks, FragT<LP> dst[P]) {
        const int s = wv + FS_NW * si;
        const ll v = v0 + st * 16;
        // 32-bit: VB * LP < 2^31 (checked by the caller), and a window
        // starts less than 64 columns past VB
        const int left = max((int)VB - (int)v, 0);
        const unsigned nrec = (unsigned)left * (LP * 2);
        #pragma unroll
        for (int p = 0; p < P; ++p) {
            const bf16_t* base = T2 + ((ll)(s * P + p) * VB + v) * LP;
            dst[p] = load_frag_buf<LP>(
                __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, nrec,
                                                  0x00020000),
                col_voff + 64u * ks);
        }
    };

    // r goes through bf16: same quantisation points as the raw-
    // correlation tensor of the streamed path.  Two per convert,
    // unpacked with a shift and a mask.
    auto quantize = [&](const f32x4 (&r)[P], f32x4 (&rq)[P]) {
        #pragma unroll
        for (int p = 0; p < P; ++p)
            #pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 pr = {r[p][2 * h], r[p][2 * h + 1]};
                unsigned u = __builtin_bit_cast(
                    unsigned, __builtin_convertvector(pr, nbf16x2));
                rq[p][2 * h] = __builtin_bit_cast(float, u << 16);
                rq[p][2 * h + 1] =
                    __builtin_bit_cast(float, u & 0xffff0000u);
            }
    };

    // 8-byte store of a task: columns st*16 + 4q .. +3 of rows (c, e),
    // e = (wv + FS_NW*si)*P + p, into the image at byte offset img.  The
    // swizzled chunk is fixed per lane and sub-tile (fcma_fused_image.h):
    // one base per sub-tile, computed once, and the rest of the address
    // is the immediate offset of the ds_write
    unsigned char* const zb = lds + TABB;
    unsigned st_base[2];
    #pragma unroll
    for (int st = 0; st < 2; ++st)
        st_base[st] = fs_img_store_base(P, wv, st, lane);
    auto store_task = [&](unsigned img, int si, int st,
                          const nbf16x4 (&zo)[P]) {
        unsigned char* dst = zb + (img + st_base[st]);
        #pragma unroll
        for (int p = 0; p < P; ++p)
            *(nbf16x4*)(dst + fs_img_store_step(P, si, p)) = zo[p];
    };

    // the wave's SPW x P (x KS) selected-voxel fragments do not depend
    // on the window: they are loaded once and stay in registers for the
    // whole sweep (16 / 32 / 64 VGPRs for LP = 16 / 32 / 64)
    FragT<LP> sel[SPW][P][KS];
    #pragma unroll
    for (int si = 0; si < SPW; ++si)
        #pragma unroll
        for (int p = 0; p < P; ++p)
            #pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                sel[si][p][ks] = load_frag<LP>(
                    sel_row((wv + FS_NW * si) * P + p), q, ks);

    // task k = 2 * si + st of the window at v0; k >= NT runs on into
    // the next window (past the last column the loads return zeros)
    auto load_task = [&](ll v0, int k, FragT<LP> dst[P]) {
        if (k >= NT) { v0 += FS_VT; k -= NT; }
        load_cols(v0, k >> 1, k & 1, 0, dst);
    };

    FragT<LP> cur[P], nxt[P];
    f32x4 rn[P];
    if (w0 < w1) {
        load_cols(w0 * FS_VT, 0, 0, 0, cur);
        if constexpr (AHEAD) {
            // cur feeds the first task's MFMAs here and is free again;
            // from now on nxt holds the columns of the task after the
            // current one and rn its correlations
            load_cols(w0 * FS_VT, 0, 1, 0, nxt);
            #pragma unroll
            for (int p = 0; p < P; ++p)
                rn[p] = corr_mfma<LP>(cur[p], sel[0][p][0], (f32x4)0.f);
        }
    }

    // What a wave does about a task whose unclamped normalize missed
    // (FORCE = false).  One-k-step instances redo the task on the spot:
    // its correlations are still in registers, one branch per task.
    // The two-k-step instances (LP = 64, 234 .. 255 VGPRs either way)
    // measured slower that way than the parent and faster this way: they
    // OR the flags of a window, and a wave with a miss redoes its own
    // tasks of that window from columns it loads again, in the phased
    // order, and overwrites its rows of the image in front of the
    // barrier.  Same MFMAs on the same operands, so the same bits.
    constexpr bool REDO_WINDOW = KS == 2;
    auto redo_window = [&](ll v0, unsigned img) {
        #pragma unroll
        for (int si = 0; si < SPW; ++si)
            #pragma unroll
            for (int st = 0; st < 2; ++st) {
                f32x4 r[P];
                #pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    FragT<LP> c[P];
                    load_cols(v0, si, st, ks, c);
                    #pragma unroll
                    for (int p = 0; p < P; ++p)
                        r[p] = corr_mfma<LP>(c[p], sel[si][p][ks],
                                             ks ? r[p] : (f32x4)0.f);
                }
                f32x4 rq[P];
                quantize(r, rq);
                nbf16x4 zo[P];
                normalize_task<P, true>(rq, zo);
                store_task(img, si, st, zo);
            }
    };

    for (ll w = w0; w < w1; ++w) {
        const ll v0 = w * FS_VT;
        const unsigned img = (unsigned)((w - w0) & 1) * fs_img_bytes();
        unsigned char* zimg = zb + img;
        // lanes whose unclamped normalize met a 1 +- r <= 0, OR-ed over
        // the tasks of the window
        unsigned long long missed = 0;
        // fully unrolled (SPW is 2 or 4) so that sel indexes statically
        #pragma unroll
        for (int si = 0; si < SPW; ++si) {
            #pragma unroll
            for (int st = 0; st < 2; ++st) {
                const int k = 2 * si + st;
                f32x4 r[P];
                if constexpr (AHEAD) {
                    // columns of task k+2 out, correlations of task
                    // k+1 out (its columns came in during task k-1),
                    // then this task's normalize on what task k-1
                    // issued.  The last tasks of the last window run
                    // on into columns nobody uses.
                    load_task(v0, k + 2, cur);
                    #pragma unroll
                    for (int p = 0; p < P; ++p) {
                        r[p] = rn[p];
                        rn[p] = corr_mfma<LP>(
                            nxt[p], sel[((k + 1) >> 1) % SPW][p][0],
                            (f32x4)0.f);
                    }
                } else {
                    // issue the next task's column loads before this
                    // task's MFMA + normalize: their latency hides
                    // under the VALU work
                    if (k + 1 < NT || w + 1 < w1) load_task(v0, k + 1, nxt);
                    #pragma unroll
                    for (int p = 0; p < P; ++p)
                        r[p] = corr_mfma<LP>(cur[p], sel[si][p][0],
                                             (f32x4)0.f);
                }
                if constexpr (KS == 2) {
                    FragT<LP> c2[P];
                    load_cols(v0, si, st, 1, c2);
                    #pragma unroll
                    for (int p = 0; p < P; ++p)
                        r[p] = corr_mfma<LP>(c2[p], sel[si][p][KS - 1],
                                             r[p]);
                }
                // Clamp found after the fact: |rq| >= 1 (the diagonal of
                // a self-correlation, duplicated voxels) is the only
                // case in which the clamp of the Fisher z changes
                // anything, and exactly there the unclamped normalize
                // ends in a NaN variance.  Nobody looks for it ahead.
                nbf16x4 zo[P];
                if constexpr (TABLE) {
                    // the lookup rounds r itself; the redo rebuilds the
                    // rounded r in the cold path
                    const unsigned long long hit =
                        normalize_task_table<P>(r, lds, zo);
                    if (__builtin_expect(hit != 0, 0)) {     // wave-uniform
                        f32x4 rq[P];
                        quantize(r, rq);
                        normalize_task<P, true>(rq, zo);
                    }
                } else {
                    f32x4 rq[P];
                    quantize(r, rq);
                    if constexpr (FORCE) {
                        normalize_task<P, true>(rq, zo);
                    } else {
                        const unsigned long long hit =
                            normalize_task<P, false>(rq, zo);
                        if constexpr (REDO_WINDOW) {
                            missed |= hit;
                        } else {
                            if (__builtin_expect(hit != 0, 0))  // uniform
                                normalize_task<P, true>(rq, zo);
                        }
                    }
                }
                store_task(img, si, st, zo);
                #pragma unroll
                for (int p = 0; p < P; ++p) {
                    if constexpr (AHEAD) nxt[p] = cur[p];
                    else cur[p] = nxt[p];
                }
            }
        }
        if constexpr (REDO_WINDOW && !FORCE) {
            if (__builtin_expect(missed != 0, 0)) redo_window(v0, img);
        }
        // window image complete.  The other buffer is free: every wave
        // passed this barrier after its Gram reads of the window before
        __syncthreads();

        #pragma unroll
        for (int i = 0; i < FS_VPW; ++i) {
            nbf16x8 f[4];
            #pragma unroll
            for (int bnd = 0; bnd < 4; ++bnd)
                f[bnd] = *(const nbf16x8*)(
                    zimg + fs_img_read_offset(wv * FS_VPW + i, bnd, lane));
            int t = 0;
            #pragma unroll
            for (int bi = 0; bi < 4; ++bi)
                #pragma unroll
                for (int bj = bi; bj < 4; ++bj, ++t)
                    G[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        f[bi], f[bj], G[i][t], 0, 0, 0);
        }
    }

    // epilogue: this block owns G (nsplit == 1, optionally shrunk the
    // way gsum_body does it) or one [count, 64, 64] partial slab
    #pragma unroll
    for (int i = 0; i < FS_VPW; ++i) {
        const ll c = c0 + wv * FS_VPW + i;
        if (c >= C) continue;                  // wave-uniform
        float scale = 1.0f;
        if (do_shrink) {
            float lead = __shfl(G[i][0][0], 0);
            lead = fmaxf(fabsf(lead), 1.0f);
            float digits = floorf(log10f(lead)) + 1.0f;
            if (digits > 2.0f)
                scale = powf(10.0f, 2.0f - digits);
        }
        float* Gc = Gout + (vs * C + c) * (ll)(FS_E * FS_E);
        const int drow = q * 4;
        int t = 0;
        #pragma unroll
        for (int bi = 0; bi < 4; ++bi)
            #pragma unroll
            for (int bj = bi; bj < 4; ++bj, ++t) {
                f32x4 val = G[i][t] * scale;
                #pragma unroll
                for (int r = 0; r < 4; ++r)
                    Gc[(bi * 16 + drow + r) * FS_E + bj * 16 + l16] =
                        val[r];
                if (bi != bj)
                    *(f32x4*)&Gc[(bj * 16 + l16) * FS_E + bi * 16 + drow]
                        = val;
            }
    }
}

static int fused_lp(ll L) {
    return L <= 16 ? 16 : (L <= 32 ? 32 : 64);
}

extern "C" int fcma_corr_gram_fused_supported(ll E, int P, ll L) {
    return E > 0 && E <= FS_E && (P == 2 || P == 4) && E % P == 0
        && L > 0 && L <= 64;
}

// row length of the cached time-contiguous layout for epoch length L
extern "C" int fcma_corr_gram_fused_lp(ll L) { return fused_lp(L); }

extern "C" int fcma_corr_gram_fused_cb(void) { return FS_CB; }
extern "C" int fcma_corr_gram_fused_vt(void) { return FS_VT; }

extern "C" void launch_fcma_corr_gram_fused(
    const void* T1, const void* T2, float* Gout, int LP, ll VA, ll VB,
    ll s0, ll C, int P, int nsplit, int do_shrink, int force_clamp,
    int schedule, int fisher, hipStream_t stream) {
    ll grid = ((C + FS_CB - 1) / FS_CB) * nsplit;
    // FS_SCHED_AUTO and FS_SCHED_AHEAD take the AHEAD order where the
    // instance has one, FS_SCHED_PHASED never does
    const bool ahead = schedule != FS_SCHED_PHASED;
    // FS_FISHER_AUTO and FS_FISHER_TABLE take the table where the
    // instance has one (fcma_corr_gram_fused_table), FS_FISHER_LOG never
    const bool table = fisher != FS_FISHER_LOG && !force_clamp;
    // force_clamp picks the instance that runs the clamped normalize for
    // every task; the other one finds the tasks that need it afterwards
    #define FS_LAUNCH_F(TP, TLP, TAHEAD, TFORCE, TTABLE)                 \
        hipLaunchKernelGGL(                                              \
            (k_corr_gram_fused<TP, TLP, TAHEAD, TFORCE, TTABLE>),        \
            dim3(grid), dim3(64 * FS_NW), 0, stream, (const bf16_t*)T1,  \
            (const bf16_t*)T2, Gout, VA, VB, s0, C, nsplit, do_shrink)
    #define FS_LAUNCH(TP, TLP, TAHEAD)                                   \
        do {                                                             \
            if constexpr (fs_has_table(TLP)) {                           \
                if (table) {                                             \
                    FS_LAUNCH_F(TP, TLP, TAHEAD, false, true);           \
                    break;                                               \
                }                                                        \
            }                                                            \
            if (force_clamp) FS_LAUNCH_F(TP, TLP, TAHEAD, true, false);  \
            else FS_LAUNCH_F(TP, TLP, TAHEAD, false, false);             \
        } while (0)
    #define FS_ONE(TP, TLP)                                              \
        do {                                                             \
            if constexpr (fs_has_ahead(TLP)) {                           \
                if (ahead) { FS_LAUNCH(TP, TLP, true); break; }          \
            }                                                            \
            FS_LAUNCH(TP, TLP, false);                                   \
        } while (0)
    if (P == 4) {
        switch (LP) {
            case 16: FS_ONE(4, 16); return;
            case 32: FS_ONE(4, 32); return;
            case 64: FS_ONE(4, 64); return;
        }
    } else if (P == 2) {
        switch (LP) {
            case 16: FS_ONE(2, 16); return;
            case 32: FS_ONE(2, 32); return;
            case 64: FS_ONE(2, 64); return;
        }
    }
    #undef FS_ONE
    #undef FS_LAUNCH
    #undef FS_LAUNCH_F
}

// whether the (P, L) instance has the AHEAD order
extern "C" int fcma_corr_gram_fused_ahead(int P, ll L) {
    (void)P;
    return fs_has_ahead(fused_lp(L));
}

// whether the (P, L) instance takes the Fisher z from the LDS table
// (clamp "auto"; the clamp "always" instances never do)
extern "C" int fcma_corr_gram_fused_table(int P, ll L) {
    (void)P;
    return fs_has_table(fused_lp(L));
}

// Tests only: the z image's layout from the functions the kernel runs
// (fcma_fused_image.h), on the host.  dims = {stride, image bytes, LDS
// bytes ahead of the first image in the table instances};
// store[wave][si][st][p][lane] (si < 64 / P / 8) and
// read[voxel][band][lane] are byte offsets into one image.
extern "C" void fcma_fused_image_layout(int P, int* dims, int* store,
                                        int* read) {
    dims[0] = (int)fs_img_stride();
    dims[1] = (int)fs_img_bytes();
    dims[2] = FS_TAB_BYTES;
    const int SPW = FS_E / P / FS_NW;
    for (int wv = 0; wv < FS_NW; ++wv)
        for (int si = 0; si < SPW; ++si)
            for (int st = 0; st < 2; ++st)
                for (int p = 0; p < P; ++p)
                    for (int lane = 0; lane < 64; ++lane)
                        *store++ = (int)fs_img_store_offset(P, wv, si, st,
                                                            p, lane);
    for (int c = 0; c < FS_CB; ++c)
        for (int bnd = 0; bnd < 4; ++bnd)
            for (int lane = 0; lane < 64; ++lane)
                *read++ = (int)fs_img_read_offset(c, bnd, lane);
}

// Tests only: the table as a workgroup builds it, and for n fp32 values
// r (bf16 patterns widened) the z of the log path and of the lookup
// (zTab[2][n]: r as the low and as the high half of a pair), through
// the device functions the kernel runs.
__global__ __launch_bounds__(64 * FS_NW) void k_fisher_table_probe(
    const float* __restrict__ r, ll n, float* __restrict__ tabOut,
    float* __restrict__ zLog, float* __restrict__ zTab) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[FS_TAB_BYTES];
    const int tid = threadIdx.x;
    fisher_table_build((float*)lds, tid, 64 * FS_NW);
    __syncthreads();
    if (blockIdx.x == 0)
        for (int i = tid; i <= FS_TAB_LAST; i += 64 * FS_NW)
            tabOut[i] = ((const float*)lds)[i];
    for (ll i = (ll)blockIdx.x * (64 * FS_NW) + tid; i < n;
         i += (ll)gridDim.x * (64 * FS_NW)) {
        // r[i] through both halves of a pair (the low half takes its
        // address from the v_mad_u32_u16, the high half from the
        // shift), each time next to another value: zTab is [2][n]
        const f32x2 r2 = {r[i], r[i]};
        const float other = r[n - 1 - i];
        zLog[i] = fisher_z_log<false>(r2)[0];
        zTab[i] = fisher_z_table((f32x2){r[i], other}, lds)[0];
        zTab[n + i] = fisher_z_table((f32x2){other, r[i]}, lds)[1];
    }
}

extern "C" int fcma_fisher_table_entries(void) { return FS_TAB_LAST + 1; }

extern "C" void launch_fcma_fisher_table_probe(
    const float* r, ll n, float* tabOut, float* zLog, float* zTab,
    hipStream_t stream) {
    const int grid = (int)min((n + 64 * FS_NW - 1) / (64 * FS_NW), (ll)64);
    hipLaunchKernelGGL(k_fisher_table_probe, dim3(max(grid, 1)),
                       dim3(64 * FS_NW), 0, stream, r, n, tabOut, zLog,
                       zTab);
}
