// Batched precomputed-kernel C-SVC cross-validation, fully on-device.
//
// The reference scores each voxel's [E,E] kernel with sklearn SVC in a CPU
// process pool (ref src/brainiak/fcma/voxelselector.py:423-465).  Here ONE
// kernel launch solves every (voxel, fold) dual QP, one wave per problem:
// SMO with maximal-violating-pair selection (LIBSVM WSS1), then the
// fold's test accuracy computed by the same wave.  VPL dual variables
// per lane: VPL=1 covers n_train <= 64, VPL=2 covers n_train <= 128
// (fp16 tile).
//
// The fp16 tile of VPL=2 holds K * 2^-qe, with qe chosen per voxel so that
// the largest |K| of the voxel's whole [E,E] matrix lands in [2^14, 2^15):
// the scale is exact, it commutes with the fp16 rounding wherever the
// unscaled value would have been a normal fp16 number, and it keeps kernels
// of any fp32 magnitude inside the fp16 range (an unscaled entry above
// 65504 would be inf, one below 6e-5 subnormal).  The solver therefore
// trains on the training block rounded to 11 significant bits and predicts
// with the unrounded fp32 rows.  Both kernels take qe from the same
// whole-matrix maximum, so their tiles hold the same values.
//
// Two kernels, identical counts:
//  - k_svm_cv: one single-wave workgroup per (voxel, fold), its own
//    signed Q tile in LDS (variable v = k*64 + lane).  Fallback for
//    E > 128 and the yardstick the shared kernel is tested against.
//  - k_svm_cv_shared (further down): one workgroup per voxel, the folds'
//    waves share one staged K tile.  The default wherever it fits.
//
// Output: correct-prediction counts [C, F] int32; host divides by test
// counts and averages folds.  The TRACE instantiations (ops.svm_cv_trace,
// for tests only) also write every test sample's decision value and each
// QP's iteration count; the production ones carry none of that code.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

typedef long long ll;

// exponent qe of the fp16 tile scale from m = max |K| of a voxel: m * 2^-qe
// lies in [2^14, 2^15).  Zero, subnormal and non-finite maxima take qe = 0.
__device__ __forceinline__ int svm_q_exponent(float m) {
    const int ex = (__float_as_int(m) >> 23) & 0xff;
    return (ex == 0 || ex == 255) ? 0 : ex - 127 - 14;
}

template <int VPL>
__device__ __forceinline__
typename std::conditional<VPL == 1, float, _Float16>::type
svm_q_enc(float x, int qe) {
    if constexpr (VPL == 1) return x;
    else return (_Float16)ldexpf(x, -qe);
}

__device__ __forceinline__ float svm_q_dec(float q, int) { return q; }
__device__ __forceinline__ float svm_q_dec(_Float16 q, int qe) {
    return ldexpf((float)q, qe);
}

__device__ __forceinline__ float wave_absmax(float mx) {
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    return mx;
}

// The two-variable instance's step arithmetic, each operation spelled out
// in the forms k_svm_cv_shared uses (see there), so that the two kernels
// agree bit for bit whatever the compiler would contract.
__device__ __forceinline__ float svm_eta2(float Qii, float Qjj, float Qij,
                                          float yi, float yj) {
    #pragma clang fp contract(off)
    return fmaf(-yj, yi * (Qij + Qij), Qii + Qjj);
}

template <bool FIRST>
__device__ __forceinline__ float svm_grad2(float g, float qi, float qj,
                                           float dai, float daj) {
    #pragma clang fp contract(off)
    float d;
    if constexpr (FIRST) d = fmaf(qi, dai, qj * daj);
    else d = qi * dai + qj * daj;
    return g + d;
}

template <int VPL, bool TRACE>
__global__ __launch_bounds__(64) void k_svm_cv(
    const float* __restrict__ kernels,  // [C, E, E]
    const float* __restrict__ y,        // [E] in {-1, +1}
    const int* __restrict__ train_idx,  // [F, E] (first n_train valid)
    const int* __restrict__ test_idx,   // [F, E] (first n_test valid)
    const int* __restrict__ n_train,    // [F]
    const int* __restrict__ n_test,     // [F]
    int* __restrict__ correct,          // [C, F]
    ll C, int E, int F, float Creg, float tol, int max_iter,
    float* __restrict__ dec_out,        // [C, F, E], TRACE only
    int* __restrict__ n_iter_out) {     // [C, F], TRACE only
    constexpr int MAXN = VPL * 64;
    const ll blk = blockIdx.x;
    const ll c = blk / F;
    const int f = (int)(blk % F);
    if (c >= C) return;
    const int lane = threadIdx.x;
    const int n = n_train[f];
    const int m = n_test[f];

    // fp32 Q for the one-variable-per-lane case; fp16 Q (0.05 % rel)
    // for n <= 128 keeps the tile at 33 KB — under the 64 KB dynamic
    // LDS launch limit and 4 QPs resident per CU
    using QT = typename std::conditional<VPL == 1, float, _Float16>::type;
    extern __shared__ char smem_raw[];
    QT (*Q)[MAXN + 1] = (QT (*)[MAXN + 1])smem_raw;
    float* ys = (float*)(smem_raw + sizeof(QT) * MAXN * (MAXN + 1));
    float* alpha_s = ys + MAXN;
    __shared__ int pair[2];
    __shared__ float delta[2];

    const float* Kc = kernels + c * (ll)E * E;
    const int* tr = train_idx + (ll)f * E;

    // fp16 tile scale from the voxel's whole matrix, as the shared kernel
    int qe = 0;
    if constexpr (VPL == 2) {
        float mx = 0.0f;
        for (int e = lane; e < E * E; e += 64)
            mx = fmaxf(mx, fabsf(Kc[e]));
        qe = __builtin_amdgcn_readfirstlane(
            svm_q_exponent(wave_absmax(mx)));
    }

    // stage labels + Q = y_i y_j K[tr_i][tr_j]
    float yl[VPL];
    #pragma unroll
    for (int k = 0; k < VPL; ++k) {
        int v = k * 64 + lane;
        yl[k] = 0.0f;
        if (v < n) {
            yl[k] = y[tr[v]];
            ys[v] = yl[k];
        }
    }
    __syncthreads();
    #pragma unroll
    for (int k = 0; k < VPL; ++k) {
        int v = k * 64 + lane;
        if (v < n) {
            const float* krow = Kc + (ll)tr[v] * E;
            for (int j = 0; j < n; ++j)
                Q[v][j] = svm_q_enc<VPL>(yl[k] * ys[j] * krow[tr[j]], qe);
        }
    }
    __syncthreads();

    // SMO: VPL dual variables per lane
    float alpha[VPL], grad[VPL];
    #pragma unroll
    for (int k = 0; k < VPL; ++k) { alpha[k] = 0.0f; grad[k] = -1.0f; }

    float b = 0.0f;
    int iters = max_iter;
    for (int iter = 0; iter < max_iter; ++iter) {
        // per-lane best over its VPL variables, then wave reduce
        float up = -3.0e38f, lo = 3.0e38f;
        int up_i = 0, lo_i = 0;
        #pragma unroll
        for (int k = 0; k < VPL; ++k) {
            int v = k * 64 + lane;
            bool valid = v < n;
            float score = -yl[k] * grad[k];
            bool in_up = valid &&
                ((yl[k] > 0.f && alpha[k] < Creg - 1e-12f) ||
                 (yl[k] < 0.f && alpha[k] > 1e-12f));
            bool in_low = valid &&
                ((yl[k] > 0.f && alpha[k] > 1e-12f) ||
                 (yl[k] < 0.f && alpha[k] < Creg - 1e-12f));
            if (in_up && score > up) { up = score; up_i = v; }
            if (in_low && score < lo) { lo = score; lo_i = v; }
        }
        #pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            float u2 = __shfl_xor(up, d);
            int ui2 = __shfl_xor(up_i, d);
            if (u2 > up) { up = u2; up_i = ui2; }
            float l2 = __shfl_xor(lo, d);
            int li2 = __shfl_xor(lo_i, d);
            if (l2 < lo) { lo = l2; lo_i = li2; }
        }
        if (up - lo < tol) {
            b = 0.5f * (up + lo);
            if constexpr (TRACE) iters = iter;
            break;
        }
        b = 0.5f * (up + lo);

        // publish lane-private alpha so lane 0 can read the pair's values
        #pragma unroll
        for (int k = 0; k < VPL; ++k) {
            int v = k * 64 + lane;
            if (v < n) alpha_s[v] = alpha[k];
        }
        __syncthreads();
        if (lane == 0) {
            int i = up_i, j = lo_i;
            float yi = ys[i], yj = ys[j];
            const float Qii = svm_q_dec(Q[i][i], qe);
            const float Qjj = svm_q_dec(Q[j][j], qe);
            const float Qij = svm_q_dec(Q[i][j], qe);
            float eta;
            if constexpr (VPL == 2) eta = svm_eta2(Qii, Qjj, Qij, yi, yj);
            else eta = Qii + Qjj - 2.0f * Qij * yi * yj;
            eta = fmaxf(eta, 1e-12f);
            float t = (up - lo) / eta;
            float ai = alpha_s[i], aj = alpha_s[j];
            float tmax_i = (yi > 0.f) ? (Creg - ai) : ai;
            float tmax_j = (yj > 0.f) ? aj : (Creg - aj);
            t = fminf(t, fminf(tmax_i, tmax_j));
            t = fmaxf(t, 0.0f);
            pair[0] = i; pair[1] = j;
            delta[0] = yi * t;      // d alpha_i
            delta[1] = -yj * t;     // d alpha_j
        }
        __syncthreads();
        const int i = pair[0], j = pair[1];
        const float dai = delta[0], daj = delta[1];
        #pragma unroll
        for (int k = 0; k < VPL; ++k) {
            int v = k * 64 + lane;
            if (v == i) alpha[k] += dai;
            if (v == j) alpha[k] += daj;
            if (v < n) {
                const float qi = svm_q_dec(Q[i][v], qe);
                const float qj = svm_q_dec(Q[j][v], qe);
                if constexpr (VPL == 2) {
                    grad[k] = k == 0
                        ? svm_grad2<true>(grad[k], qi, qj, dai, daj)
                        : svm_grad2<false>(grad[k], qi, qj, dai, daj);
                } else {
                    grad[k] += qi * dai + qj * daj;
                }
            }
        }
        __syncthreads();
    }

    // publish final alpha, predict test samples
    #pragma unroll
    for (int k = 0; k < VPL; ++k) {
        int v = k * 64 + lane;
        if (v < n) alpha_s[v] = alpha[k] * yl[k];  // coef_i = alpha_i y_i
    }
    __syncthreads();
    const int* te = test_idx + (ll)f * E;
    int correct_local = 0;
    #pragma unroll
    for (int k = 0; k < VPL; ++k) {
        int v = k * 64 + lane;
        if (v < m) {
            const float* krow = Kc + (ll)te[v] * E;
            float dec = b;
            for (int i = 0; i < n; ++i)
                dec = fmaf(alpha_s[i], krow[tr[i]], dec);
            float yt = y[te[v]];
            correct_local += ((dec > 0.f) == (yt > 0.f)) ? 1 : 0;
            if constexpr (TRACE)
                dec_out[((ll)c * F + f) * E + v] = dec;
        }
    }
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        correct_local += __shfl_xor(correct_local, d);
    if (lane == 0) {
        correct[c * F + f] = correct_local;
        if constexpr (TRACE) n_iter_out[c * F + f] = iters;
    }
}

// ---------------------------------------------------------------------------
// Shared-tile variant: one workgroup per VOXEL, one wave per fold.
//
// The four (F) folds of a voxel solve QPs over sub-matrices of the same
// [E,E] kernel, so the block stages K once (row stride S = E|1, fp32 for
// VPL=1, fp16 for VPL=2) and every fold-wave reads it:
// Q[i][v] = (y_i y_v) K[tr_i][tr_v], the +-1 sign applied on the fly
// (exact, and it commutes with the fp16 rounding, so the values are the
// ones k_svm_cv stores).  After the staging barrier the waves never meet
// again: a QP is one wave, its trip count is its own, and there is NO
// block barrier below that line.
//
// An SMO iteration touches LDS once (the two Q rows, independent reads):
//  - lane l owns variable bitrev6(l) (+64 for the second one), so that
//    "first set bit of the (score == best) ballot" is exactly the winner
//    of k_svm_cv's strict-compare xor butterfly as lane 0 sees it (the
//    tied lane with the smallest bit-reversed index; a lane's k=0
//    candidate beats its k=1 on ties).  The value itself is reduced with
//    DPP max/min and then re-read from the winning lane, so a -0/+0 tie
//    returns the winner's zero as the butterfly does.
//  - every lane computes the step from v_readlane of the pair's y,
//    alpha, row offset and diagonal; Q_ij is lane j's element of row i.
//
// The arithmetic forms are those k_svm_cv compiles to (contraction is off
// here and each fma is spelled out), so the two variants give the same
// trajectory bit for bit: eta = fma(-y_j, y_i*(Q_ij+Q_ij), Q_ii+Q_jj);
// correctly rounded division; grad + (Q_iv*da_i + Q_jv*da_j) unfused,
// except the FIRST variable of a two-variable lane, which k_svm_cv<2>
// computes as grad + fma(Q_iv, da_i, Q_jv*da_j) (svm_grad2 above).

// order-preserving float <-> int32 key (its own inverse): the reduction
// runs on integers, so the DPP operand folds into v_max_i32/v_min_i32
// and no NaN-quieting canonicalisation sits between the steps.  Scores
// are never NaN here (a candidate passed an ordered compare), and -0
// and +0 get adjacent keys, which the float == ballot treats as a tie.
__device__ __forceinline__ int float_key(int bits) {
    return bits ^ ((bits >> 31) & 0x7fffffff);
}

template <bool IS_MAX>
__device__ __forceinline__ float wave_reduce_dpp(float xf) {
    // quad xor 1, quad xor 2, half-row mirror, row mirror, then the two
    // row broadcasts: lane 63 ends up holding the wave's max/min
    int x = float_key(__float_as_int(xf));
#define SVM_DPP_STEP(ctrl, row_mask)                                        \
    {                                                                       \
        int o = __builtin_amdgcn_update_dpp(                                \
            IS_MAX ? (int)0x80000000 : 0x7fffffff, x, ctrl, row_mask, 0xf,  \
            false);  /* rows masked off see the identity */                 \
        x = IS_MAX ? max(x, o) : min(x, o);                                 \
    }
    SVM_DPP_STEP(0xB1, 0xf)    // quad_perm [1,0,3,2]
    SVM_DPP_STEP(0x4E, 0xf)    // quad_perm [2,3,0,1]
    SVM_DPP_STEP(0x141, 0xf)   // row_half_mirror
    SVM_DPP_STEP(0x140, 0xf)   // row_mirror
    SVM_DPP_STEP(0x142, 0xa)   // row_bcast:15 into rows 1, 3
    SVM_DPP_STEP(0x143, 0xc)   // row_bcast:31 into rows 2, 3
#undef SVM_DPP_STEP
    return __int_as_float(float_key(__builtin_amdgcn_readlane(x, 63)));
}

__device__ __forceinline__ float lane_f(float x, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

__device__ __forceinline__ int first_lane(unsigned long long m) {
    return m ? (int)__ffsll((long long)m) - 1 : 0;
}

template <int VPL, bool TRACE>
__global__ __launch_bounds__(512) void k_svm_cv_shared(
    const float* __restrict__ kernels,  // [C, E, E]
    const float* __restrict__ y,        // [E] in {-1, +1}
    const int* __restrict__ train_idx,  // [F, E] (first n_train valid)
    const int* __restrict__ test_idx,   // [F, E] (first n_test valid)
    const int* __restrict__ n_train,    // [F]
    const int* __restrict__ n_test,     // [F]
    int* __restrict__ correct,          // [C, F]
    ll C, int E, int F, int S, float Creg, float tol, int max_iter,
    float* __restrict__ dec_out,        // [C, F, E], TRACE only
    int* __restrict__ n_iter_out) {     // [C, F], TRACE only
    #pragma clang fp contract(off)
    using QT = typename std::conditional<VPL == 1, float, _Float16>::type;
    extern __shared__ char smem_raw[];
    QT* tile = (QT*)smem_raw;           // [E][S], K as given (no sign)

    const ll c = blockIdx.x;
    if (c >= C) return;                 // whole block: before the barrier
    const float* Kc = kernels + c * (ll)E * E;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int EE = E * E;

    // fp16 tile scale from the voxel's whole matrix, as k_svm_cv<2>
    int qe = 0;
    if constexpr (VPL == 2) {
        __shared__ float wmax[8];
        float mx = 0.0f;
        for (int e = tid; e < EE; e += nthr)
            mx = fmaxf(mx, fabsf(Kc[e]));
        mx = wave_absmax(mx);
        if ((tid & 63) == 0) wmax[tid >> 6] = mx;
        __syncthreads();
        mx = wmax[0];
        for (int w = 1; w < (nthr >> 6); ++w) mx = fmaxf(mx, wmax[w]);
        qe = __builtin_amdgcn_readfirstlane(svm_q_exponent(mx));
    }

    // stage K once for all folds: 16-byte coalesced loads when the
    // voxel's matrix is 16-byte aligned (E even and an aligned base)
    int done = 0;
    if ((((uintptr_t)Kc) & 15) == 0) {
        const int nvec = EE >> 2;
        for (int q = tid; q < nvec; q += nthr) {
            const float4 v4 = ((const float4*)Kc)[q];
            const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
            int r = (q * 4) / E;
            int cc = q * 4 - r * E;
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                tile[r * S + cc] = svm_q_enc<VPL>(vv[u], qe);
                if (++cc == E) { cc = 0; ++r; }
            }
        }
        done = nvec << 2;
    }
    for (int e = done + tid; e < EE; e += nthr) {
        int r = e / E;
        tile[r * S + (e - r * E)] = svm_q_enc<VPL>(Kc[e], qe);
    }
    __syncthreads();
    // ---- no block-level barrier from here on ----

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwave = nthr >> 6;
    const int lane = tid & 63;
    const int vb = (int)(__brev((unsigned)lane) >> 26);   // bitrev6(lane)
    const float cup = Creg - 1e-12f;

    for (int f = wave; f < F; f += nwave) {
        const int n = n_train[f];
        const int m = n_test[f];
        const int* tr = train_idx + (ll)f * E;
        const int* te = test_idx + (ll)f * E;

        // lane-private variables: v = k*64 + bitrev6(lane)
        bool valid[VPL];
        int col[VPL];                   // tr[v]: column (and row) in K
        float yl[VPL], qd[VPL], alpha[VPL], grad[VPL];
        #pragma unroll
        for (int k = 0; k < VPL; ++k) {
            int v = k * 64 + vb;
            valid[k] = v < n;
            col[k] = valid[k] ? tr[v] : 0;
            yl[k] = valid[k] ? y[col[k]] : 0.0f;
            // Q_vv = K_vv
            qd[k] = svm_q_dec(tile[col[k] * S + col[k]], qe);
            alpha[k] = 0.0f;
            grad[k] = -1.0f;
        }

        float b = 0.0f;
        int iters = max_iter;
        for (int iter = 0; iter < max_iter; ++iter) {
            // per-lane best over its VPL variables (k=0 wins ties)
            float uv = -3.0e38f, lv = 3.0e38f;
            int ku = 0, kl = 0;
            #pragma unroll
            for (int k = 0; k < VPL; ++k) {
                float score = -yl[k] * grad[k];
                bool in_up = valid[k] &&
                    ((yl[k] > 0.f && alpha[k] < cup) ||
                     (yl[k] < 0.f && alpha[k] > 1e-12f));
                bool in_low = valid[k] &&
                    ((yl[k] > 0.f && alpha[k] > 1e-12f) ||
                     (yl[k] < 0.f && alpha[k] < cup));
                if (in_up && score > uv) { uv = score; ku = k; }
                if (in_low && score < lv) { lv = score; kl = k; }
            }
            // value by DPP, index = first lane holding it (bit-reversed
            // layout => the butterfly's winner); no candidate anywhere
            // leaves every lane at the sentinel and picks variable 0
            const float ubest = wave_reduce_dpp<true>(uv);
            const float lbest = wave_reduce_dpp<false>(lv);
            const int li = first_lane(__ballot(uv == ubest));
            const int lj = first_lane(__ballot(lv == lbest));
            const float up = lane_f(uv, li);
            const float lo = lane_f(lv, lj);
            const float gap = __fsub_rn(up, lo);
            b = __fmul_rn(0.5f, __fadd_rn(up, lo));
            if (gap < tol) {
                if constexpr (TRACE) iters = iter;
                break;
            }

            // each lane's own candidate, then the pair's via readlane
            float yu = yl[0], au = alpha[0], du = qd[0];
            float ylo = yl[0], alo = alpha[0], dlo = qd[0];
            int cu = col[0], clo = col[0];
            if (VPL == 2) {
                if (ku) { yu = yl[VPL - 1]; au = alpha[VPL - 1];
                          du = qd[VPL - 1]; cu = col[VPL - 1]; }
                if (kl) { ylo = yl[VPL - 1]; alo = alpha[VPL - 1];
                          dlo = qd[VPL - 1]; clo = col[VPL - 1]; }
            }
            const float yi = lane_f(yu, li), yj = lane_f(ylo, lj);
            const float ai = lane_f(au, li), aj = lane_f(alo, lj);
            const float Qii = lane_f(du, li), Qjj = lane_f(dlo, lj);
            const int ri = __builtin_amdgcn_readlane(cu, li) * S;
            const int rj = __builtin_amdgcn_readlane(clo, lj) * S;
            const int ki = __builtin_amdgcn_readlane(ku, li);
            const int kj = __builtin_amdgcn_readlane(kl, lj);

            // the iteration's only LDS traffic: rows i and j
            float qi[VPL], qj[VPL];
            #pragma unroll
            for (int k = 0; k < VPL; ++k) {
                float a = svm_q_dec(tile[ri + col[k]], qe);
                float bq = svm_q_dec(tile[rj + col[k]], qe);
                qi[k] = __fmul_rn(__fmul_rn(yi, yl[k]), a);
                qj[k] = __fmul_rn(__fmul_rn(yj, yl[k]), bq);
            }
            float qsel = qi[0];
            if (VPL == 2 && kl) qsel = qi[VPL - 1];
            const float Qij = lane_f(qsel, lj);

            float eta = fmaf(-yj, __fmul_rn(yi, __fadd_rn(Qij, Qij)),
                             __fadd_rn(Qii, Qjj));
            eta = fmaxf(eta, 1e-12f);
            float t = __fdiv_rn(gap, eta);
            float tmax_i = (yi > 0.f) ? __fsub_rn(Creg, ai) : ai;
            float tmax_j = (yj > 0.f) ? aj : __fsub_rn(Creg, aj);
            t = fminf(t, fminf(tmax_i, tmax_j));
            t = fmaxf(t, 0.0f);
            const float dai = __fmul_rn(yi, t);      // d alpha_i
            const float daj = __fmul_rn(-yj, t);     // d alpha_j

            #pragma unroll
            for (int k = 0; k < VPL; ++k) {
                if (lane == li && k == ki) alpha[k] = __fadd_rn(alpha[k], dai);
                if (lane == lj && k == kj) alpha[k] = __fadd_rn(alpha[k], daj);
                float d;
                if (VPL == 2 && k == 0)
                    d = fmaf(qi[k], dai, __fmul_rn(qj[k], daj));
                else
                    d = __fadd_rn(__fmul_rn(qi[k], dai),
                                  __fmul_rn(qj[k], daj));
                if (valid[k]) grad[k] = __fadd_rn(grad[k], d);
            }
        }

        // predict the fold's test samples: the sequential fmaf chain
        // over variables 0..n-1, coefficients and columns by readlane.
        // All lanes walk the chain (idle ones on row 0) so the readlane
        // sources stay active.  VPL=1 reads K from the tile; the fp16
        // tile of VPL=2 is not what k_svm_cv predicts with, so that
        // instance reads the fp32 matrix from global memory as it does.
        float coef[VPL];
        #pragma unroll
        for (int k = 0; k < VPL; ++k)
            coef[k] = __fmul_rn(alpha[k], yl[k]);   // coef_i = alpha_i y_i
        int correct_w = 0;
        #pragma unroll
        for (int k = 0; k < VPL; ++k) {
            if (k * 64 >= m) break;
            const int tv = k * 64 + lane;
            const bool act = tv < m;
            const int trow = act ? te[tv] : 0;
            const float yt = y[trow];
            float dec = b;
            #pragma unroll
            for (int kk = 0; kk < VPL; ++kk) {
                const int cnt = min(64, n - kk * 64);
                for (int i = 0; i < cnt; ++i) {
                    const int src = (int)(__brev((unsigned)i) >> 26);
                    const float cf = lane_f(coef[kk], src);
                    const int ci = __builtin_amdgcn_readlane(col[kk], src);
                    float kv;
                    if (VPL == 1) kv = (float)tile[trow * S + ci];
                    else          kv = Kc[(ll)trow * E + ci];
                    dec = fmaf(cf, kv, dec);
                }
            }
            correct_w += __popcll(__ballot(
                act && ((dec > 0.f) == (yt > 0.f))));
            if constexpr (TRACE)
                if (act) dec_out[(c * F + f) * E + tv] = dec;
        }
        if (lane == 0) {
            correct[c * F + f] = correct_w;
            if constexpr (TRACE) n_iter_out[c * F + f] = iters;
        }
    }
}

// tile bytes of the shared variant, or 0 when the shape is not covered.
// The tile is the whole [E, E] matrix (k_svm_cv stages only a fold's
// [n, n] part) and must fit the 64 KB dynamic-LDS launch limit.  E is
// capped at 128, the range the equality tests cover; an fp16 tile of a
// larger E could still fit, but those shapes stay on k_svm_cv.
static size_t svm_cv_shared_smem(int E, ll max_n) {
    if (E < 1 || E > 128 || max_n < 1 || max_n > 128) return 0;
    size_t bytes = (size_t)E * (size_t)(E | 1) * (max_n <= 64 ? 4 : 2);
    return bytes <= 65536 ? bytes : 0;
}

extern "C" int svm_cv_shared_fits(int E, ll max_n) {
    return svm_cv_shared_smem(E, max_n) != 0;
}

// variant: 0 = auto (shared when it fits), 1 = shared, 2 = one wave per QP
template <bool TRACE>
static void launch_svm_cv_t(const float* kernels, const float* y,
                            const int* train_idx, const int* test_idx,
                            const int* n_train, const int* n_test,
                            int* correct, float* dec, int* n_iter, ll C,
                            int E, int F, float Creg, float tol,
                            int max_iter, ll max_n, int variant,
                            hipStream_t stream) {
    const size_t shared_smem = svm_cv_shared_smem(E, max_n);
    if (variant != 2 && shared_smem != 0) {
        const int W = F < 8 ? F : 8;
        const int S = E | 1;
        if (max_n <= 64)
            hipLaunchKernelGGL((k_svm_cv_shared<1, TRACE>),
                               dim3((unsigned)C), dim3(64 * W), shared_smem,
                               stream, kernels, y, train_idx, test_idx,
                               n_train, n_test, correct, C, E, F, S, Creg,
                               tol, max_iter, dec, n_iter);
        else
            hipLaunchKernelGGL((k_svm_cv_shared<2, TRACE>),
                               dim3((unsigned)C), dim3(64 * W), shared_smem,
                               stream, kernels, y, train_idx, test_idx,
                               n_train, n_test, correct, C, E, F, S, Creg,
                               tol, max_iter, dec, n_iter);
        return;
    }
    if (max_n <= 64) {
        size_t smem = (size_t)64 * 65 * 4 + 2 * 64 * 4;
        hipLaunchKernelGGL((k_svm_cv<1, TRACE>), dim3((unsigned)(C * F)),
                           dim3(64), smem, stream, kernels, y, train_idx,
                           test_idx, n_train, n_test, correct, C, E, F,
                           Creg, tol, max_iter, dec, n_iter);
        return;
    }
    size_t smem = (size_t)128 * 129 * 2 + 2 * 128 * 4;   // fp16 Q
    hipLaunchKernelGGL((k_svm_cv<2, TRACE>), dim3((unsigned)(C * F)),
                       dim3(64), smem, stream, kernels, y, train_idx,
                       test_idx, n_train, n_test, correct, C, E, F, Creg,
                       tol, max_iter, dec, n_iter);
}

extern "C" void launch_svm_cv(const float* kernels, const float* y,
                              const int* train_idx, const int* test_idx,
                              const int* n_train, const int* n_test,
                              int* correct, ll C, int E, int F, float Creg,
                              float tol, int max_iter, ll max_n,
                              int variant, hipStream_t stream) {
    launch_svm_cv_t<false>(kernels, y, train_idx, test_idx, n_train, n_test,
                           correct, nullptr, nullptr, C, E, F, Creg, tol,
                           max_iter, max_n, variant, stream);
}

// the same launch through the TRACE instantiations: dec [C, F, E] fp32 and
// n_iter [C, F] int32 are written next to the counts (tests only)
extern "C" void launch_svm_cv_trace(const float* kernels, const float* y,
                                    const int* train_idx,
                                    const int* test_idx, const int* n_train,
                                    const int* n_test, int* correct,
                                    float* dec, int* n_iter, ll C, int E,
                                    int F, float Creg, float tol,
                                    int max_iter, ll max_n, int variant,
                                    hipStream_t stream) {
    launch_svm_cv_t<true>(kernels, y, train_idx, test_idx, n_train, n_test,
                          correct, dec, n_iter, C, E, F, Creg, tol,
                          max_iter, max_n, variant, stream);
}
