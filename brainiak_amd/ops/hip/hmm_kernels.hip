// Log-space HMM forward-backward for EventSegment's left-to-right event
// chains (MI355X counterpart of the recursion the reference keeps in
// eventseg/event.py:284-369 with its native helper eventseg/_utils.pyx),
// and, further down, the MAP event path over the same graph
// (k_hmm_viterbi).
//
// The transition graph is sparse: every event state k has a self loop
// (log_self[k]) and at most one outgoing edge to succ[k] (log_adv[k]);
// the absorbing sink never carries mass in either pass (its observation
// column is -inf and log_end[sink] = -inf), so only the K event states
// are computed.  With lae(x, y) = log(exp(x) + exp(y)):
//
//   alpha_0[k] = log_start[k] + lp[0,k]
//   alpha_t[k] = lae(alpha_{t-1}[k] + log_self[k],
//                    alpha_{t-1}[pred[k]] + log_adv[pred[k]]) + lp[t,k]
//   ll         = logsumexp_k(alpha_{T-1}[k] + log_end[k])
//   beta_{T-1}[k] = log_end[k]
//   w[k]       = beta_{t+1}[k] + lp[t+1,k]
//   beta_t[k]  = lae(log_self[k] + w[k], log_adv[k] + w[succ[k]])
//   log_gamma[t,k] = alpha_t[k] + beta_t[k]
//                    - logsumexp_k(alpha_t[k] + beta_t[k])
//
// One block = one wave (64 threads) per sequence b; lane k < K owns state
// k, and the pred/succ exchange is a cross-lane gather (__shfl), so chains
// may interleave arbitrarily.  Everything is fp64.
//
// The T recursion is a serial dependency chain, so no global access sits
// inside it.  lp streams through in tiles of HMM_TT timesteps: a [TT, K]
// slab is contiguous in [B, T, K], all 64 lanes load it coalesced into
// registers one tile AHEAD of use (the loads are in flight while the
// current tile is consumed), and it is handed to the owning lanes through
// LDS at the tile boundary.  Results go the same way back: the step loop
// writes LDS, the whole tile is stored coalesced after it.
//
// In place: the forward pass writes alpha into the log_gamma buffer; the
// backward pass streams alpha[t,k] back (same tiling) and overwrites it
// with log_gamma[t,k].  No alpha/beta/sink-padded temporaries exist.
//
// HMM_TT = 16: the backward pass holds two tiles in LDS (lp and alpha),
// 2 * 16 * K * 8 B = 16 KiB at K = 64 (dynamic, sized by the real K: 2 KiB
// at K = 8), so ten K=64 waves still fit the 160 KiB of a CU — more than
// the 4 SIMDs need for this ALU-bound fp64 chain — and the prefetch costs
// at most 2 * 16 doubles = 64 VGPRs per lane.  One step is a few hundred
// fp64 instructions (exp + log1p), so a 16-step tile spans many times the
// HBM latency the prefetch has to cover; larger tiles would only spend
// LDS and registers.

#include <hip/hip_runtime.h>

typedef long long ll;

#define HMM_TT 16
#define HMM_MAXK 64

extern "C" int hmm_fb_tile(void) { return HMM_TT; }

__device__ __forceinline__ double hmm_neg_inf() {
    return -__builtin_huge_val();
}

// log(exp(x) + exp(y)); -inf (not NaN) when both are -inf
__device__ __forceinline__ double hmm_lae(double x, double y) {
    double m = fmax(x, y);
    double r = m + log1p(exp(-fabs(x - y)));
    return (m == hmm_neg_inf()) ? m : r;
}

// logsumexp over the 64 lanes (lanes >= K carry -inf)
__device__ __forceinline__ double hmm_wave_lse(double s) {
    double m = s;
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        m = fmax(m, __shfl_xor(m, d));
    if (m == hmm_neg_inf()) return m;      // wave-uniform
    double e = (s == hmm_neg_inf()) ? 0.0 : exp(s - m);
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        e += __shfl_xor(e, d);
    return m + log(e);
}

// coalesced slab load into registers: element i = r * 64 + lane, i < n
__device__ __forceinline__ void hmm_load_tile(double (&reg)[HMM_TT],
                                              const double* src, int n,
                                              int lane) {
    #pragma unroll
    for (int r = 0; r < HMM_TT; ++r) {
        int i = r * 64 + lane;
        if (i < n) reg[r] = src[i];
    }
}

__device__ __forceinline__ void hmm_regs_to_lds(const double (&reg)[HMM_TT],
                                                double* dst, int n,
                                                int lane) {
    #pragma unroll
    for (int r = 0; r < HMM_TT; ++r) {
        int i = r * 64 + lane;
        if (i < n) dst[i] = reg[r];
    }
}

__device__ __forceinline__ void hmm_lds_to_global(const double* src,
                                                  double* dst, int n,
                                                  int lane) {
    #pragma unroll
    for (int r = 0; r < HMM_TT; ++r) {
        int i = r * 64 + lane;
        if (i < n) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(64) void k_hmm_fb(
    const double* __restrict__ lp,        // [B, T, K]
    const double* __restrict__ log_start, // [K]
    const double* __restrict__ log_end,   // [K]
    const double* __restrict__ log_self,  // [K]
    const double* __restrict__ log_adv,   // [K]
    const int* __restrict__ pred,         // [K], -1 = chain head
    const int* __restrict__ succ,         // [K], -1 = chain tail
    double* __restrict__ out,             // [B, T, K] alpha, then log_gamma
    double* __restrict__ ll_out,          // [B]
    ll B, int T, int K) {
    const ll b = blockIdx.x;
    if (b >= B) return;
    const int k = threadIdx.x;
    const bool live = k < K;

    extern __shared__ double hmm_sm[];
    double* sA = hmm_sm;                  // [TT, K] alpha / log_gamma tile
    double* sL = hmm_sm + HMM_TT * K;     // [TT, K] lp tile (backward)

    const double ninf = hmm_neg_inf();
    // dead lanes (k >= K) hold -inf everywhere and never feed a live lane
    const double l_start = live ? log_start[k] : ninf;
    const double l_end = live ? log_end[k] : ninf;
    const double l_self = live ? log_self[k] : 0.0;
    const double l_adv = live ? log_adv[k] : ninf;
    int p = live ? pred[k] : -1;
    int s = live ? succ[k] : -1;
    const bool has_p = p >= 0 && p < K;
    const bool has_s = s >= 0 && s < K;
    p = has_p ? p : k;
    s = has_s ? s : k;

    const double* lpb = lp + b * (ll)T * K;
    double* ob = out + b * (ll)T * K;
    const int ntiles = (T + HMM_TT - 1) / HMM_TT;

    double rL[HMM_TT], rA[HMM_TT];

    // ---- forward: alpha into the output buffer ------------------------
    double a = ninf;
    hmm_load_tile(rL, lpb, min(HMM_TT, T) * K, k);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int t0 = tile * HMM_TT;
        const int nt = min(HMM_TT, T - t0);
        const int n = nt * K;
        __syncthreads();                  // previous tile's LDS reads done
        hmm_regs_to_lds(rL, sA, n, k);
        __syncthreads();
        if (tile + 1 < ntiles)            // next slab in flight from here
            hmm_load_tile(rL, lpb + (ll)(t0 + HMM_TT) * K,
                          min(HMM_TT, T - t0 - HMM_TT) * K, k);
        for (int tt = 0; tt < nt; ++tt) {
            const double x = live ? sA[tt * K + k] : 0.0;
            if (t0 + tt == 0) {
                a = l_start + x;
            } else {
                double v = __shfl(a + l_adv, p);
                v = has_p ? v : ninf;
                a = hmm_lae(a + l_self, v) + x;
            }
            if (live) sA[tt * K + k] = a;
        }
        __syncthreads();
        hmm_lds_to_global(sA, ob + (ll)t0 * K, n, k);
    }
    {
        const double l = hmm_wave_lse(a + l_end);
        if (k == 0) ll_out[b] = l;
    }

    // alpha was stored by other lanes of this wave: make it visible
    // before the backward pass streams it back
    __threadfence();
    __syncthreads();

    // ---- backward: beta on the fly, log_gamma over alpha --------------
    double w = ninf;                      // beta_{t+1} + lp[t+1]
    {
        const int t0 = (ntiles - 1) * HMM_TT;
        const int n = (T - t0) * K;
        hmm_load_tile(rL, lpb + (ll)t0 * K, n, k);
        hmm_load_tile(rA, ob + (ll)t0 * K, n, k);
    }
    for (int tile = ntiles - 1; tile >= 0; --tile) {
        const int t0 = tile * HMM_TT;
        const int nt = min(HMM_TT, T - t0);
        const int n = nt * K;
        __syncthreads();
        hmm_regs_to_lds(rL, sL, n, k);
        hmm_regs_to_lds(rA, sA, n, k);
        __syncthreads();
        if (tile > 0) {                   // full tiles only below the last
            hmm_load_tile(rL, lpb + (ll)(t0 - HMM_TT) * K, HMM_TT * K, k);
            hmm_load_tile(rA, ob + (ll)(t0 - HMM_TT) * K, HMM_TT * K, k);
        }
        for (int tt = nt - 1; tt >= 0; --tt) {
            double beta;
            if (t0 + tt == T - 1) {
                beta = l_end;
            } else {
                double v = __shfl(w, s);
                v = has_s ? l_adv + v : ninf;
                beta = hmm_lae(l_self + w, v);
            }
            const double x = live ? sL[tt * K + k] : 0.0;
            const double al = live ? sA[tt * K + k] : ninf;
            const double g = al + beta;
            const double z = hmm_wave_lse(g);
            if (live) sA[tt * K + k] = g - z;
            w = beta + x;
        }
        __syncthreads();
        hmm_lds_to_global(sA, ob + (ll)t0 * K, n, k);
    }
}

// ---------------------------------------------------------------------------
// MAP event path (Viterbi) over the same chain graph: the max-plus twin of
// the forward pass above, same wave/lane map and the same lp streaming.
//
//   d_0[k]    = log_start[k] + lp[0,k]
//   vs        = d_{t-1}[k] + log_self[k]
//   va        = d_{t-1}[pred[k]] + log_adv[pred[k]]     (-inf at a head)
//   take_t[k] = pred[k] >= 0 and va > vs      (ties keep the self loop)
//   d_t[k]    = (take_t[k] ? va : vs) + lp[t,k]
//   final     = lowest k maximising d_{T-1}[k] + log_end[k]; score = max
//   path[T-1] = final; path[t-1] = take_t[path[t]] ? pred[path[t]] : path[t]
//
// Only fp64 additions and comparisons, in exactly this order, so the result
// is bit-identical to the torch recursion in EventSegment._viterbi_batch.
//
// A state has one possible predecessor besides itself, so the back-pointers
// of a timestep are one bit per state: __ballot(take) is the whole step.
// Lane (t & 63) keeps the mask of step t in a register; every HMM_VT = 64
// steps the wave stores its 64 masks coalesced into the [B, T] int64
// scratch.  No delta is ever written.  The backtrace reads the masks back
// in the same 64-step tiles, one coalesced load each (L2 hits: the wave
// wrote them moments ago).  Lane j reads the very word it wrote, so the
// round trip needs no fence.  The walk itself is
// scalar: the current state is wave-uniform, the step's mask and pred[state]
// come from v_readlane, and lane j records the state at step t0 + j for one
// coalesced int32 store per tile.

#define HMM_VT 64

extern "C" int hmm_viterbi_tile(void) { return HMM_VT; }

__global__ __launch_bounds__(64) void k_hmm_viterbi(
    const double* __restrict__ lp,        // [B, T, K]
    const double* __restrict__ log_start, // [K]
    const double* __restrict__ log_end,   // [K]
    const double* __restrict__ log_self,  // [K]
    const double* __restrict__ log_adv,   // [K]
    const int* __restrict__ pred,         // [K], -1 = chain head
    ll* __restrict__ masks,               // [B, T] scratch, bit k = take_t[k]
    int* __restrict__ path,               // [B, T]
    double* __restrict__ score,           // [B]
    ll B, int T, int K) {
    const ll b = blockIdx.x;
    if (b >= B) return;
    const int k = threadIdx.x;
    const bool live = k < K;

    extern __shared__ double hmm_sm[];
    double* sL = hmm_sm;                  // [TT, K] lp tile

    const double ninf = hmm_neg_inf();
    const double l_start = live ? log_start[k] : ninf;
    const double l_end = live ? log_end[k] : ninf;
    const double l_self = live ? log_self[k] : 0.0;
    const double l_adv = live ? log_adv[k] : ninf;
    const int p_raw = live ? pred[k] : -1;
    const bool has_p = p_raw >= 0 && p_raw < K;
    const int p = has_p ? p_raw : k;

    const double* lpb = lp + b * (ll)T * K;
    ll* mb = masks + b * (ll)T;
    int* pb = path + b * (ll)T;
    const int ntiles = (T + HMM_TT - 1) / HMM_TT;

    double rL[HMM_TT];

    // ---- forward: max-plus recursion, one mask word per step ----------
    double d = ninf;
    ll m = 0;                             // mask of step (t & 63) == k
    hmm_load_tile(rL, lpb, min(HMM_TT, T) * K, k);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int t0 = tile * HMM_TT;
        const int nt = min(HMM_TT, T - t0);
        __syncthreads();                  // previous tile's LDS reads done
        hmm_regs_to_lds(rL, sL, nt * K, k);
        __syncthreads();
        if (tile + 1 < ntiles)            // next slab in flight from here
            hmm_load_tile(rL, lpb + (ll)(t0 + HMM_TT) * K,
                          min(HMM_TT, T - t0 - HMM_TT) * K, k);
        // HMM_TT divides 64: a tile never straddles a mask word's lanes
        const int j0 = t0 & (HMM_VT - 1);
        #pragma unroll
        for (int tt = 0; tt < HMM_TT; ++tt) {
            if (tt < nt) {                // wave-uniform
                const double x = live ? sL[tt * K + k] : 0.0;
                ll mask = 0;
                if (t0 + tt == 0) {
                    d = l_start + x;
                } else {
                    const double vs = d + l_self;
                    double va = __shfl(d + l_adv, p);
                    va = has_p ? va : ninf;
                    const bool take = has_p && va > vs;
                    mask = (ll)__ballot(take);
                    d = (take ? va : vs) + x;
                }
                if (k == j0 + tt) m = mask;
            }
        }
        const int tend = t0 + nt;
        if ((tend & (HMM_VT - 1)) == 0 || tile == ntiles - 1) {
            const int base = (tend - 1) & ~(HMM_VT - 1);
            if (base + k < tend) mb[base + k] = m;
        }
    }

    // ---- final state: lowest k at the maximum -------------------------
    const double f = d + l_end;
    double best = f;
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        best = fmax(best, __shfl_xor(best, o));
    // lane 0 is always live, and all -inf still compares equal
    const unsigned long long at_best = __ballot(live && f == best);
    int s = __builtin_amdgcn_readfirstlane(__ffsll((long long)at_best) - 1);
    if (k == 0) score[b] = best;

    // ---- backtrace: read the masks back, walk a uniform state ---------
    const int nbt = (T + HMM_VT - 1) / HMM_VT;
    for (int bt = nbt - 1; bt >= 0; --bt) {
        const int t0 = bt * HMM_VT;
        const int nt = min(HMM_VT, T - t0);
        ll cur = 0;
        if (k < nt) cur = mb[t0 + k];     // this lane's own store
        const int cur_lo = (int)(cur & 0xffffffffLL);
        const int cur_hi = (int)(cur >> 32);
        int mine = 0;
        for (int j = nt - 1; j >= 0; --j) {
            if (k == j) mine = s;         // path[t0 + j]
            // the mask of step 0 is 0: the state stays put below t = 0
            const int w = __builtin_amdgcn_readlane(s < 32 ? cur_lo : cur_hi,
                                                    j);
            const int ps = __builtin_amdgcn_readlane(p_raw, s);
            s = ((w >> (s & 31)) & 1) ? ps : s;
        }
        if (k < nt) pb[t0 + k] = mine;
    }
}

extern "C" void launch_hmm_viterbi(const double* lp, const double* log_start,
                                   const double* log_end,
                                   const double* log_self,
                                   const double* log_adv, const int* pred,
                                   ll* masks, int* path, double* score,
                                   ll B, int T, int K, hipStream_t stream) {
    const size_t smem = (size_t)HMM_TT * K * sizeof(double);
    hipLaunchKernelGGL(k_hmm_viterbi, dim3((unsigned)B), dim3(64), smem,
                       stream, lp, log_start, log_end, log_self, log_adv,
                       pred, masks, path, score, B, T, K);
}

extern "C" void launch_hmm_fb(const double* lp, const double* log_start,
                              const double* log_end, const double* log_self,
                              const double* log_adv, const int* pred,
                              const int* succ, double* out, double* ll_out,
                              ll B, int T, int K, hipStream_t stream) {
    const size_t smem = (size_t)2 * HMM_TT * K * sizeof(double);
    hipLaunchKernelGGL(k_hmm_fb, dim3((unsigned)B), dim3(64), smem, stream,
                       lp, log_start, log_end, log_self, log_adv, pred,
                       succ, out, ll_out, B, T, K);
}
