// Gather-and-summarise for the resampling nulls of the ISC statistics
// (bootstrap_isc, permutation_isc, timeshift_isc in brainiak_amd/isc.py);
// further down, contract-and-summarise for the phase-randomisation null
// (phaseshift_isc), which shares the statistics.
//
// Every leave-one-out and pairwise variant of the subject bootstrap, the
// sign-flip and label-shuffle permutation tests and the circular time-shift
// test does the same thing per draw i and voxel v:
//
//   x_r      = signs[i,r] * table[rows[i,r], lags[i,r], v]      r = 0..R-1
//   out[i,v] = stat over the r with signs[i,r] != 0 and x_r not NaN
//
// with stat = 'median' (numpy's nanmedian: the middle value, or (a + b) / 2
// of the two middle values for an even count) or 'mean' (the Fisher mean
// tanh(mean(atanh(x))), atanh results that are NaN skipped as nanmean does,
// so atanh(+-1) = +-inf survives and a lone +1 gives exactly 1.0).  No
// surviving value gives NaN.  The table is fp64 [N, L, V] with V innermost:
// L = 1 for bootstrap / permutation (rows of ISC values), L = T for the
// time-shift test (all T circular lags of every subject).
//
// Mapping.  One block = one wave = 64 consecutive voxels of one draw; lane
// = voxel, so every gathered row segment is one coalesced 512-B read.  The
// grid is 1-D, block = draw * nTiles + tile (tile fastest: neighbouring
// blocks read neighbouring segments of the same table rows).  The (row,
// lag, sign) triples of a draw depend on blockIdx only, so they are
// wave-uniform scalar loads, and the row base is scalar arithmetic in 64
// bits: ((ll)row * L + lag) * V.  The r loop is unrolled by ISC_UNROLL = 4
// with the four loads issued before the first use, so four independent row
// reads are in flight per wave.
//
// Median.  Each lane keeps its column sorted in LDS, laid out [R][lane]:
// element j of lane l sits at byte (j * 64 + l) * 8, so whatever j each
// lane is at, the 64 lanes of an access touch consecutive 8-byte words
// (bank (2 l) mod 64: lanes l and l + 32 share a bank but sit in different
// halves of a ds_read_b64 / ds_write_b64, which are served separately) -
// conflict-free although the insert position differs per lane.  Selection
// is an online insertion sort while gathering: a surviving value is
// shifted in from the top of the lane's sorted prefix (strict >, so equal
// values keep their order).  It is exact, needs no sentinel for the entries
// left out, and costs about R^2 / 4 LDS read+write pairs per output, which
// at the R <= 32 of real subject counts is of the order of the gather
// itself.  At the end the lane reads its middle element(s).
//
// LDS budget.  R * 64 lanes * 8 B = 512 R bytes per wave, allocated
// dynamically by the real R: 16 KiB at R = 32 (ten waves per 160-KiB CU),
// and ISC_MAX_ROWS = 128 gives 64 KiB, the largest dynamic allocation that
// needs no per-kernel opt-in, still two waves per CU.  128 rows cover
// leave-one-out up to 128 subjects and pairwise up to 16 subjects (120
// pairs).  Larger R takes the caller's torch path.  'mean' needs no
// storage and has no cap.
//
// fp64 throughout, no fast-math, no atomics.  The caller has checked that
// every row is in [0, N) and every lag in [0, L).

#include <hip/hip_runtime.h>

typedef long long ll;

#define ISC_MAX_ROWS 128
#define ISC_UNROLL 4

extern "C" int isc_resample_max_rows(void) { return ISC_MAX_ROWS; }

__device__ __forceinline__ double isc_nan() {
    return __builtin_nan("");
}

// shift x into the lane's sorted column col[0 .. n) (stride 64 doubles)
__device__ __forceinline__ void isc_insert(double* col, int& n, double x) {
    if (x == x) {
        int j = n;
        while (j > 0) {
            const double y = col[(j - 1) * 64];
            if (!(y > x)) break;
            col[j * 64] = y;
            --j;
        }
        col[j * 64] = x;
        ++n;
    }
}

struct IscMeanAcc {
    double sum;
    int n;
};

__device__ __forceinline__ void isc_accumulate(IscMeanAcc& acc, double x) {
    const double z = atanh(x);
    if (z == z) {
        acc.sum += z;
        ++acc.n;
    }
}

template <bool MEDIAN>
__global__ __launch_bounds__(64) void k_isc_resample_stat(
    const double* __restrict__ table,      // [N, L, V]
    const int* __restrict__ rows,          // [I, R]
    const int* __restrict__ lags,          // [I, R] or null (all zero)
    const signed char* __restrict__ signs, // [I, R]
    double* __restrict__ out,              // [I, V]
    ll L, ll V, int R, int nTiles) {
    const int tile = (int)(blockIdx.x % (unsigned)nTiles);
    const ll i = (ll)(blockIdx.x / (unsigned)nTiles);
    const int lane = threadIdx.x;
    const ll v = (ll)tile * 64 + lane;
    const bool live = v < V;

    extern __shared__ double isc_sm[];
    double* col = isc_sm + lane;           // [R][64], this lane's column

    const int* rw = rows + i * R;
    const int* lg = lags ? lags + i * R : nullptr;
    const signed char* sg = signs + i * R;

    int n = 0;                             // median: values in the column
    IscMeanAcc acc = {0.0, 0};

    for (int r0 = 0; r0 < R; r0 += ISC_UNROLL) {
        double x[ISC_UNROLL];
        int s[ISC_UNROLL];
        // issue the row reads of this group before any of them is used;
        // an entry that its sign leaves out is read all the same (its
        // indices are in range too), so no read waits for a sign byte
        #pragma unroll
        for (int u = 0; u < ISC_UNROLL; ++u) {
            const int r = r0 + u;
            s[u] = 0;
            x[u] = isc_nan();
            if (r < R) {                   // wave-uniform
                s[u] = sg[r];
                const ll base = ((ll)rw[r] * L + (lg ? lg[r] : 0)) * V;
                if (live) x[u] = table[base + v];
            }
        }
        #pragma unroll
        for (int u = 0; u < ISC_UNROLL; ++u) {
            if (s[u] != 0) {               // wave-uniform; 0 leaves it out
                const double xs = (double)s[u] * x[u];
                if (MEDIAN) isc_insert(col, n, xs);
                else isc_accumulate(acc, xs);
            }
        }
    }

    if (!live) return;
    double res = isc_nan();
    if (MEDIAN) {
        if (n > 0) {
            const double hi = col[(n >> 1) * 64];
            res = hi;
            if ((n & 1) == 0) res = (col[((n >> 1) - 1) * 64] + hi) / 2.0;
        }
    } else {
        if (acc.n > 0) res = tanh(acc.sum / (double)acc.n);
    }
    out[i * V + v] = res;
}

extern "C" void launch_isc_resample_stat(const double* table, const int* rows,
                                         const int* lags,
                                         const signed char* signs,
                                         double* out, ll I, ll L, ll V,
                                         int R, int median,
                                         hipStream_t stream) {
    const ll nTiles = (V + 63) / 64;
    const dim3 grid((unsigned)(I * nTiles));
    if (median) {
        const size_t smem = (size_t)R * 64 * sizeof(double);
        hipLaunchKernelGGL(k_isc_resample_stat<true>, grid, dim3(64), smem,
                           stream, table, rows, lags, signs, out, L, V, R,
                           (int)nTiles);
    } else {
        hipLaunchKernelGGL(k_isc_resample_stat<false>, grid, dim3(64), 0,
                           stream, table, rows, lags, signs, out, L, V, R,
                           (int)nTiles);
    }
}

// ---------------------------------------------------------------------------
// Contract-and-summarise for the phase-randomisation null (phaseshift_isc).
//
// The correlation of a phase-randomised series with a fixed one is linear in
// the cosines and sines of the drawn phases, so per draw i, row r (subject or
// pair) and voxel v
//
//   x[i,r,v] = sum_k coef[i,r,k] * table[r,k,v]              k = 0..K-1
//   out[i,v] = stat over the r with x[i,r,v] not NaN
//
// with the statistics of k_isc_resample_stat above.  table is fp64 [R, K, V]
// (V innermost), coef fp64 [I, R, K]; a NaN in the table reaches x through
// the product.  The [I, R, V] intermediate never leaves the registers: when
// a row's sum is complete it goes straight into the lane's sorted LDS column
// (median) or the Fisher accumulator (mean).
//
// Mapping.  One block = one wave = 64 consecutive voxels of D consecutive
// draws; lane = voxel, so every table read is one coalesced 512-B segment
// and is used for D FMAs.  The grid is 1-D, block = tile * nDrawTiles +
// drawTile (draw tile fastest): the blocks that share a voxel tile, and so
// the same R * K * 512-B slice of the table, are neighbours and find it in
// L2.  coef depends on the block and on (r, k) only: wave-uniform scalar
// loads, the FMAs take them as scalar operands.  Rows r and columns k are
// contiguous in both arrays, so the table is one stream of J = R * K
// segments; segment j starts at j * V, formed in 64 bits from two 32-bit
// factors (the caller checks J and V), a wave-uniform base that the lane's
// own 32-bit offset is added to.
//
// The stream is read in groups of ISC_PHASE_UNROLL = 8 segments that are
// aligned to the rows (a row's last group may be partly used).  Two register
// sets alternate: the eight reads of the next group are issued before the
// 8 * D FMAs of the current one, so no read is waited for where it is
// issued and no set is copied.  Reads are never predicated: a segment index
// past the end is clamped to the last segment and a lane past V reads the
// last voxel; what they fetch is not used.
//
// Draw tile and LDS.  Median storage is one sorted column per lane and draw
// of the tile, D * R * 512 bytes, within the same 64 KiB of dynamic LDS as
// above: D = 4 up to R = 32, D = 2 up to R = 64, D = 1 up to R =
// ISC_MAX_ROWS = 128; more rows take the caller's torch path.  'mean' needs
// no storage: D = 8 for any R.  A tile that reaches past the last draw
// computes the last draw again in its surplus slots and does not store them.
//
// fp64 throughout (one fused multiply-add per term, in k order), no
// fast-math, no atomics.  The caller guarantees K >= 1, R >= 1.

#define ISC_PHASE_UNROLL 8
#define ISC_PHASE_MEAN_DRAWS 8

extern "C" int isc_phase_max_rows(void) { return ISC_MAX_ROWS; }

// draws per block of the median path for R rows (R <= ISC_MAX_ROWS)
static int isc_phase_median_draws(int R) {
    return R <= 32 ? 4 : (R <= 64 ? 2 : 1);
}

// segment j (clamped into the stream) of this lane's voxel
__device__ __forceinline__ double isc_phase_load(const double* tb, int j,
                                                 int J, unsigned V,
                                                 unsigned lv) {
    const int jj = j < J ? j : J - 1;
    return (tb + (unsigned long long)(unsigned)jj * V)[lv];
}

// One group of the stream: issue the reads of the next group into nxt, add
// the current group's terms (cur) to the row sums s, and when the group ends
// its row hand the sums to the statistic.  (r, k0) is the group's position
// and is advanced to the next group's.
template <bool MEDIAN, int D>
__device__ __forceinline__ void isc_phase_group(
    const double (&cur)[ISC_PHASE_UNROLL], double (&nxt)[ISC_PHASE_UNROLL],
    double (&s)[D], int (&n)[D], IscMeanAcc (&acc)[D],
    const double* const (&cf)[D], const double* tb, double* col0,
    int& r, int& k0, int R, int K, int J, unsigned V, unsigned lv) {
    constexpr int U = ISC_PHASE_UNROLL;
    const bool last = k0 + U >= K;         // this group ends its row
    const int rn = last ? r + 1 : r;
    const int kn = last ? 0 : k0 + U;
    const int jn = rn * K + kn;            // J after the last group
    #pragma unroll
    for (int u = 0; u < U; ++u) nxt[u] = isc_phase_load(tb, jn + u, J, V, lv);

    const int jc = r * K + k0;
    if (k0 + U <= K) {
        #pragma unroll
        for (int u = 0; u < U; ++u) {
            #pragma unroll
            for (int d = 0; d < D; ++d)
                s[d] = fma(cf[d][jc + u], cur[u], s[d]);
        }
    } else if (D <= 4) {
        // a row's partly used last group: all its coefficients are asked
        // for at once (clamped, like the reads), then the terms in range
        // are added - with few waves per CU a scalar load waited for inside
        // each guarded term would not be hidden
        double c[D][U];
        #pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jj = jc + u < J ? jc + u : J - 1;
            #pragma unroll
            for (int d = 0; d < D; ++d) c[d][u] = cf[d][jj];
        }
        #pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + u < K) {              // wave-uniform
                #pragma unroll
                for (int d = 0; d < D; ++d)
                    s[d] = fma(c[d][u], cur[u], s[d]);
            }
        }
    } else {
        #pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + u < K) {              // wave-uniform
                #pragma unroll
                for (int d = 0; d < D; ++d)
                    s[d] = fma(cf[d][jc + u], cur[u], s[d]);
            }
        }
    }

    if (last) {
        #pragma unroll
        for (int d = 0; d < D; ++d) {
            if (MEDIAN) isc_insert(col0 + (ll)d * R * 64, n[d], s[d]);
            else isc_accumulate(acc[d], s[d]);
            s[d] = 0.0;
        }
    }
    r = rn;
    k0 = kn;
}

template <bool MEDIAN, int D>
__global__ __launch_bounds__(64) void k_isc_phase_stat(
    const double* __restrict__ table,      // [R, K, V]
    const double* __restrict__ coef,       // [I, R, K]
    double* __restrict__ out,              // [I, V]
    ll I, int V, int R, int K, int nDrawTiles) {
    constexpr int U = ISC_PHASE_UNROLL;
    const int tile = (int)(blockIdx.x / (unsigned)nDrawTiles);
    const ll i0 = (ll)(blockIdx.x % (unsigned)nDrawTiles) * D;
    const int lane = threadIdx.x;
    const int v0 = tile * 64;
    const bool live = v0 + lane < V;
    const int J = R * K;                   // segments in the stream

    extern __shared__ double isc_sm[];     // median: [D][R][64]
    double* col0 = isc_sm + lane;

    // the tile's voxels in segment 0 (wave-uniform) and this lane's offset
    // (a lane past V reads the last voxel)
    const double* tb = table + v0;
    const unsigned lv = live ? (unsigned)lane : (unsigned)(V - 1 - v0);
    // coefficient rows of the tile's draws (past I: the last draw again)
    const double* cf[D];
    #pragma unroll
    for (int d = 0; d < D; ++d) {
        const ll id = i0 + d < I ? i0 + d : I - 1;
        cf[d] = coef + id * J;
    }

    double s[D];                           // sums of the row in progress
    int n[D];                              // median: values in each column
    IscMeanAcc acc[D];
    #pragma unroll
    for (int d = 0; d < D; ++d) {
        s[d] = 0.0;
        n[d] = 0;
        acc[d].sum = 0.0;
        acc[d].n = 0;
    }

    double xa[U], xb[U];
    #pragma unroll
    for (int u = 0; u < U; ++u)
        xa[u] = isc_phase_load(tb, u, J, (unsigned)V, lv);

    const int G = R * ((K + U - 1) / U);   // groups in the stream
    int r = 0, k0 = 0;
    for (int g = 0; g < G; g += 2) {
        isc_phase_group<MEDIAN, D>(xa, xb, s, n, acc, cf, tb, col0, r, k0, R,
                                   K, J, (unsigned)V, lv);
        if (g + 1 >= G) break;
        isc_phase_group<MEDIAN, D>(xb, xa, s, n, acc, cf, tb, col0, r, k0, R,
                                   K, J, (unsigned)V, lv);
    }

    if (!live) return;
    #pragma unroll
    for (int d = 0; d < D; ++d) {
        if (i0 + d >= I) break;            // wave-uniform
        double res = isc_nan();
        if (MEDIAN) {
            const double* col = col0 + (ll)d * R * 64;
            if (n[d] > 0) {
                const double hi = col[(n[d] >> 1) * 64];
                res = hi;
                if ((n[d] & 1) == 0)
                    res = (col[((n[d] >> 1) - 1) * 64] + hi) / 2.0;
            }
        } else {
            if (acc[d].n > 0) res = tanh(acc[d].sum / (double)acc[d].n);
        }
        out[(i0 + d) * V + v0 + lane] = res;
    }
}

template <bool MEDIAN, int D>
static void isc_phase_launch(const double* table, const double* coef,
                             double* out, ll I, ll V, int R, int K,
                             hipStream_t stream) {
    const ll nTiles = (V + 63) / 64;
    const ll nDrawTiles = (I + D - 1) / D;
    const dim3 grid((unsigned)(nTiles * nDrawTiles));
    const size_t smem = MEDIAN ? (size_t)D * R * 64 * sizeof(double) : 0;
    hipLaunchKernelGGL((k_isc_phase_stat<MEDIAN, D>), grid, dim3(64), smem,
                       stream, table, coef, out, I, (int)V, R, K,
                       (int)nDrawTiles);
}

// blocks of one launch, for the caller's range check
extern "C" ll isc_phase_blocks(ll I, ll V, int R, int median) {
    const int D = median ? isc_phase_median_draws(R) : ISC_PHASE_MEAN_DRAWS;
    return ((V + 63) / 64) * ((I + D - 1) / D);
}

extern "C" void launch_isc_phase_stat(const double* table, const double* coef,
                                      double* out, ll I, ll V, int R, int K,
                                      int median, hipStream_t stream) {
    if (!median) {
        isc_phase_launch<false, ISC_PHASE_MEAN_DRAWS>(table, coef, out, I, V,
                                                      R, K, stream);
        return;
    }
    switch (isc_phase_median_draws(R)) {
    case 4:
        isc_phase_launch<true, 4>(table, coef, out, I, V, R, K, stream);
        break;
    case 2:
        isc_phase_launch<true, 2>(table, coef, out, I, V, R, K, stream);
        break;
    default:
        isc_phase_launch<true, 1>(table, coef, out, I, V, R, K, stream);
    }
}
