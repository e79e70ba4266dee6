// Gather-and-summarise for the resampling nulls of the ISC statistics
// (bootstrap_isc, permutation_isc, timeshift_isc in brainiak_amd/isc.py).
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
