// Per-centre Gram matrices of searchlight activity vectors.
//
// The activity-based voxel selector scores every searchlight with a
// linear SVM, which needs only the [E, E] Gram of the ball's voxels:
//
//   G_c[e, e'] = sum over v in shape(c) & mask of x[v, e] * x[v, e']
//
// x [B, X, Y, Z, E] fp32 (epoch innermost), mask [B, X, Y, Z] uint8,
// shape [K, K, K] uint8 (K = 2 rad + 1 <= 9), centres [N] int64 linear
// voxel indices into [B, X, Y, Z]; every centre lies at least rad from
// each block face (checked on the host, never here).  G [N, E, E] fp32.
//
// One 256-thread workgroup per centre:
//  1. the four waves ballot-compact the K^3 offsets with shape & mask
//     set into an LDS list, in ascending offset order (nv <= 729), so
//     the summation order is fixed;
//  2. the listed voxel rows stream through LDS in slabs of 32 rows of
//     Epad = 16 NT floats (E rounded up to a tile; pad rows and pad
//     columns are zero).  The next slab's rows are fetched into
//     registers while the current one is multiplied;
//  3. the NT (NT + 1) / 2 upper-triangular 16x16 tiles are dealt round
//     robin to the waves.  Each wave keeps its tiles' accumulators in
//     registers over all slabs and feeds v_mfma_f32_16x16x4_f32 (exact
//     fp32, an fmaf chain over the voxels) from one LDS read per tile
//     row and k-step: the A and the B operand of a Gram are the same
//     fragments;
//  4. upper tiles are written with their mirror image, diagonal tiles
//     write only row <= col and mirror it, so G == G^T bit for bit.
//
// The kernel is instantiated per NT (1..16, E <= 256) and per wave so
// that every accumulator index is a compile-time constant.  The LDS row
// stride is Epad or Epad + 16, whichever is 16 or 48 mod 64: the four
// voxel rows of one MFMA operand read then fall into disjoint banks.
// Every index into x, mask and G is 64-bit.

#include <hip/hip_runtime.h>

typedef long long ll;
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SG_THREADS 256
#define SG_WAVES 4
#define SG_SLAB 32           // voxel rows per LDS slab
#define SG_MAX_K3 729        // 9^3
#define SG_ROUNDS 3          // ceil(729 / 256)
#define SG_MAX_NT 16         // E <= 256

extern "C" int sl_gram_max_e(void) { return 16 * SG_MAX_NT; }

template <int NT>
struct SgShape {
    static constexpr int EPAD = 16 * NT;
    static constexpr int STRIDE = (NT & 1) ? EPAD : EPAD + 16;
    static constexpr int TILES = NT * (NT + 1) / 2;
    static constexpr int TPW = (TILES + SG_WAVES - 1) / SG_WAVES;
    static constexpr int QUADS = SG_SLAB * EPAD / 4;       // per slab
    static constexpr int QPT = (QUADS + SG_THREADS - 1) / SG_THREADS;
    static constexpr int KSTEP_UNROLL = NT <= 4 ? SG_SLAB / 4 : 1;
};

// index of upper tile (ti, tj), tj >= ti, in row-major upper order
__host__ __device__ constexpr int sg_tile_id(int nt, int ti, int tj) {
    return ti * nt - ti * (ti - 1) / 2 + (tj - ti);
}

// One slab of MFMAs for wave W: 8 k-steps of 4 voxel rows.
template <int NT, int W>
__device__ __forceinline__ void sg_mma(const float* slab, int lane,
                                       f32x4 (&acc)[SgShape<NT>::TPW]) {
    constexpr int S = SgShape<NT>::STRIDE;
    const float* p0 = slab + (lane >> 4) * S + (lane & 15);
    // few tiles per wave: unroll the k-steps so that the LDS reads of
    // the next step overlap the MFMAs; many tiles: one step already
    // holds enough MFMAs, and unrolling only costs registers (104 + 36
    // against 54 + 36 VGPRs + AGPRs at NT = 8)
    #pragma unroll SgShape<NT>::KSTEP_UNROLL
    for (int step = 0; step < SG_SLAB / 4; ++step) {
        const float* p = p0 + step * 4 * S;
        float a[NT];
        #pragma unroll
        for (int i = 0; i < NT; ++i) a[i] = p[16 * i];
        #pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            #pragma unroll
            for (int tj = ti; tj < NT; ++tj) {
                const int t = sg_tile_id(NT, ti, tj);
                if (t % SG_WAVES == W)
                    acc[t / SG_WAVES] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a[ti], a[tj], acc[t / SG_WAVES], 0, 0, 0);
            }
        }
    }
}

// Write wave W's tiles and their mirror images.
template <int NT, int W>
__device__ __forceinline__ void sg_store(float* Gc, int E, int lane,
                                         const f32x4 (&acc)[SgShape<NT>::TPW]) {
    const int dcol = lane & 15;
    const int drow = (lane >> 4) * 4;
    const bool vec = (E & 3) == 0;
    #pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        #pragma unroll
        for (int tj = ti; tj < NT; ++tj) {
            const int t = sg_tile_id(NT, ti, tj);
            if (t % SG_WAVES != W) continue;
            const f32x4 v = acc[t / SG_WAVES];
            const int row0 = 16 * ti + drow;
            const int col = 16 * tj + dcol;
            if (col >= E) continue;
            if (ti != tj) {
                #pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (row0 + r < E) Gc[(ll)(row0 + r) * E + col] = v[r];
                if (vec) {
                    // row0 % 4 == 0 and E % 4 == 0: all four rows live
                    if (row0 < E)
                        *reinterpret_cast<f32x4*>(Gc + (ll)col * E + row0) = v;
                } else {
                    #pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row0 + r < E)
                            Gc[(ll)col * E + row0 + r] = v[r];
                }
            } else {
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + r;
                    if (row <= col) {
                        Gc[(ll)row * E + col] = v[r];
                        Gc[(ll)col * E + row] = v[r];
                    }
                }
            }
        }
    }
}

template <int NT>
__global__ __launch_bounds__(SG_THREADS) void k_sl_gram(
    const float* __restrict__ x, const unsigned char* __restrict__ mask,
    const unsigned char* __restrict__ shape, const ll* __restrict__ centres,
    float* __restrict__ G, int Y, int Z, int E, int K) {
    typedef SgShape<NT> SH;
    constexpr int S = SH::STRIDE;

    __shared__ __attribute__((aligned(16))) float slab[SG_SLAB * S];
    __shared__ int list[SG_ROUNDS * SG_THREADS];
    __shared__ int wcnt[SG_ROUNDS][SG_WAVES];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const ll n = blockIdx.x;
    const ll c0 = centres[n];

    // ---- 1. ordered compaction of the live offsets ---------------------
    const int rad = K >> 1;
    const int K3 = K * K * K;
    int rel[SG_ROUNDS];
    unsigned long long bal[SG_ROUNDS];
    bool live[SG_ROUNDS];
    #pragma unroll
    for (int i = 0; i < SG_ROUNDS; ++i) {
        const int idx = i * SG_THREADS + tid;
        live[i] = false;
        rel[i] = 0;
        if (idx < K3) {
            const int d = idx % K;
            const int b = (idx / K) % K;
            const int a = idx / (K * K);
            rel[i] = ((a - rad) * Y + (b - rad)) * Z + (d - rad);
            live[i] = shape[idx] != 0 && mask[c0 + rel[i]] != 0;
        }
        bal[i] = __ballot(live[i]);
        if (lane == 0) wcnt[i][w] = __popcll(bal[i]);
    }
    __syncthreads();
    int nv = 0;
    #pragma unroll
    for (int i = 0; i < SG_ROUNDS; ++i) {
        #pragma unroll
        for (int ww = 0; ww < SG_WAVES; ++ww) {
            if (ww == w && live[i])
                list[nv + __popcll(bal[i] & ((1ull << lane) - 1ull))]
                    = rel[i];
            nv += wcnt[i][ww];
        }
    }
    __syncthreads();

    // ---- 2./3. stream the rows, accumulate the tiles -------------------
    const bool vec = (E & 3) == 0;
    f32x4 pf[SH::QPT];
    auto fetch = [&](int s) {
        #pragma unroll
        for (int j = 0; j < SH::QPT; ++j) {
            const int q = j * SG_THREADS + tid;
            f32x4 v = (f32x4)0.f;
            if (q < SH::QUADS) {
                const int row = q / (SH::EPAD / 4);
                const int c = (q % (SH::EPAD / 4)) * 4;
                const int vi = s * SG_SLAB + row;
                if (vi < nv && c < E) {
                    const float* src = x + (c0 + list[vi]) * (ll)E + c;
                    if (vec) {
                        v = *reinterpret_cast<const f32x4*>(src);
                    } else {
                        v[0] = src[0];
                        if (c + 1 < E) v[1] = src[1];
                        if (c + 2 < E) v[2] = src[2];
                        if (c + 3 < E) v[3] = src[3];
                    }
                }
            }
            pf[j] = v;
        }
    };
    auto stage = [&]() {
        #pragma unroll
        for (int j = 0; j < SH::QPT; ++j) {
            const int q = j * SG_THREADS + tid;
            if (q < SH::QUADS) {
                const int row = q / (SH::EPAD / 4);
                const int c = (q % (SH::EPAD / 4)) * 4;
                *reinterpret_cast<f32x4*>(&slab[row * S + c]) = pf[j];
            }
        }
    };

    f32x4 acc[SH::TPW];
    #pragma unroll
    for (int i = 0; i < SH::TPW; ++i) acc[i] = (f32x4)0.f;

    const int nslab = (nv + SG_SLAB - 1) / SG_SLAB;
    if (nslab > 0) fetch(0);
    for (int s = 0; s < nslab; ++s) {
        stage();
        __syncthreads();
        if (s + 1 < nslab) fetch(s + 1);
        switch (w) {
            case 0: sg_mma<NT, 0>(slab, lane, acc); break;
            case 1: sg_mma<NT, 1>(slab, lane, acc); break;
            case 2: sg_mma<NT, 2>(slab, lane, acc); break;
            default: sg_mma<NT, 3>(slab, lane, acc); break;
        }
        __syncthreads();
    }

    // ---- 4. both triangles ---------------------------------------------
    float* Gc = G + n * (ll)E * E;
    switch (w) {
        case 0: sg_store<NT, 0>(Gc, E, lane, acc); break;
        case 1: sg_store<NT, 1>(Gc, E, lane, acc); break;
        case 2: sg_store<NT, 2>(Gc, E, lane, acc); break;
        default: sg_store<NT, 3>(Gc, E, lane, acc); break;
    }
}

template <int NT>
static void sg_launch(const float* x, const unsigned char* mask,
                      const unsigned char* shape, const ll* centres,
                      float* G, ll N, int Y, int Z, int E, int K,
                      hipStream_t stream) {
    hipLaunchKernelGGL((k_sl_gram<NT>), dim3((unsigned)N), dim3(SG_THREADS),
                       0, stream, x, mask, shape, centres, G, Y, Z, E, K);
}

extern "C" void launch_sl_gram(const float* x, const unsigned char* mask,
                               const unsigned char* shape,
                               const ll* centres, float* G, ll N, int Y,
                               int Z, int E, int K, hipStream_t stream) {
#define SG_CASE(nt) \
    case nt: sg_launch<nt>(x, mask, shape, centres, G, N, Y, Z, E, K, \
                           stream); break;
    switch ((E + 15) / 16) {
        SG_CASE(1) SG_CASE(2) SG_CASE(3) SG_CASE(4) SG_CASE(5) SG_CASE(6)
        SG_CASE(7) SG_CASE(8) SG_CASE(9) SG_CASE(10) SG_CASE(11)
        SG_CASE(12) SG_CASE(13) SG_CASE(14) SG_CASE(15) SG_CASE(16)
        default: break;   // E above the cap: rejected by the binding
    }
#undef SG_CASE
}
