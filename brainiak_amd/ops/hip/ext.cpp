// Torch bindings for the brainiak_amd HIP/CDNA4 kernels (gfx950).
//
// The device code lives in fcma_kernels.hip / procrustes.hip /
// tfa_kernels.hip / hmm_kernels.hip / isc_stats_kernels.hip /
// isc_corr_kernels.hip (hand-written
// HIP, MFMA/LDS — no library GEMMs on the FCMA path); this file validates
// tensors, allocates outputs, and calls the extern "C" launchers on the
// current stream.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <climits>
#include <string>

#include "fcma_launch.h"   // everything fcma_kernels.hip exports

typedef long long ll;

// the other kernel files' launchers (void* stands in for hipStream_t)
extern "C" {
void launch_jacobi_eigh(const float*, float*, float*, ll, int, void*);
void launch_tfa_factor(const float*, const float*, const float*, float*,
                       ll, int, void*);
void launch_tfa_recon(const float*, const float*, const float*, float*,
                      ll, ll, int, float, void*);
void launch_svm_cv(const float*, const float*, const int*, const int*,
                   const int*, const int*, int*, ll, int, int, float,
                   float, int, ll, int, void*);
int svm_cv_shared_fits(int, ll);
void launch_svm_cv_trace(const float*, const float*, const int*, const int*,
                         const int*, const int*, int*, float*, int*, ll,
                         int, int, float, float, int, ll, int, void*);
void launch_isfc_accum(float*, const void*, ll, ll, int, void*);
void launch_isfc_fused(float*, const void*, const void*, ll, ll, ll,
                       void*);
void launch_stencil3d(const float*, const float*, float*, ll, int, int,
                      int, int, void*);
int fcma_corr_gram_fused_supported(ll, int, ll);
int fcma_corr_gram_fused_lp(ll);
int fcma_corr_gram_fused_cb(void);
int fcma_corr_gram_fused_vt(void);
int fcma_corr_gram_fused_ahead(int, ll);
int fcma_corr_gram_fused_table(int, ll);
void launch_fcma_corr_gram_fused(const void*, const void*, float*, int, ll,
                                 ll, ll, ll, int, int, int, int, int, int,
                                 void*);
void fcma_fused_image_layout(int, int*, int*, int*);
int fcma_fisher_table_entries(void);
void launch_fcma_fisher_table_probe(const float*, ll, float*, float*,
                                    float*, void*);
void launch_hmm_fb(const double*, const double*, const double*,
                   const double*, const double*, const int*, const int*,
                   double*, double*, ll, int, int, void*);
int hmm_fb_tile(void);
void launch_hmm_viterbi(const double*, const double*, const double*,
                        const double*, const double*, const int*, ll*,
                        int*, double*, ll, int, int, void*);
int hmm_viterbi_tile(void);
void launch_isc_resample_stat(const double*, const int*, const int*,
                              const signed char*, double*, ll, ll, ll, int,
                              int, void*);
int isc_resample_max_rows(void);
void launch_isc_phase_stat(const double*, const double*, double*, ll, ll,
                           int, int, int, void*);
int isc_phase_max_rows(void);
ll isc_phase_blocks(ll, ll, int, int);
void launch_isc_loo(const double*, double*, int*, double*, unsigned char*,
                    ll, ll, ll, int, int, double, void*);
ll isc_loo_blocks(ll, ll, int);
void launch_isc_pairwise(const double*, double*, unsigned char*, ll, ll, ll,
                         int, double, void*);
ll isc_pairwise_blocks(ll, int);
int isc_pairwise_max_subjects(void);
void launch_sl_gram(const float*, const unsigned char*,
                    const unsigned char*, const ll*, float*, ll, int, int,
                    int, int, void*);
int sl_gram_max_e(void);
}

static hipStream_t cur_stream() {
    return at::cuda::getCurrentCUDAStream().stream();
}

static void check_3d(const torch::Tensor& t, c10::ScalarType dt,
                     const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.dim() == 3, name, " must be 3-D");
    TORCH_CHECK(t.scalar_type() == dt, name, " has wrong dtype");
}

// ---------------------------------------------------------------------------

torch::Tensor fcma_normalize_(torch::Tensor corr, int64_t P) {
    check_3d(corr, torch::kFloat32, "corr");
    ll C = corr.size(0), E = corr.size(1), V = corr.size(2);
    TORCH_CHECK(P > 0 && E % P == 0, "epochs_per_subj must divide E");
    launch_fcma_normalize(corr.data_ptr<float>(), C, E, V, (int)P,
                          cur_stream());
    return corr;
}

static const char* const kBadL =
    "epoch length must be padded to one of {8,12,16,20,24,28,32,36,40}";
// a (P, L)-templated launcher found no instantiation and launched nothing
static const char* const kNoKernel =
    "no FCMA kernel instantiation for this shape: ";

static int pick_p_for_raw(ll E) {
    for (int p : {8, 4, 2}) if (E % p == 0) return p;
    return 1;
}

torch::Tensor fcma_correlate(torch::Tensor A, torch::Tensor B,
                             int64_t start, int64_t count) {
    check_3d(A, torch::kBFloat16, "A");
    check_3d(B, torch::kBFloat16, "B");
    ll E = A.size(0), L = A.size(1), VA = A.size(2), VB = B.size(2);
    TORCH_CHECK(B.size(0) == E && B.size(1) == L, "A/B epoch shapes differ");
    TORCH_CHECK(start >= 0 && start + count <= VA, "voxel range");
    TORCH_CHECK(fcma_supported_L(L) == L, kBadL);
    int P = pick_p_for_raw(E);
    auto out = torch::empty({count, E, VB},
                            A.options().dtype(torch::kFloat32));
    TORCH_CHECK(launch_fcma_corr_norm(A.data_ptr(), B.data_ptr(), nullptr,
                                      out.data_ptr<float>(), E, L, VA, VB,
                                      start, count, P, /*mode=*/2, E,
                                      cur_stream(), nullptr),
                kNoKernel, "P=", P, " L=", L);
    return out;
}

torch::Tensor fcma_corr_norm_z(torch::Tensor A, torch::Tensor B,
                               int64_t start, int64_t count, int64_t P,
                               int64_t padE,
                               c10::optional<torch::Tensor> out_opt,
                               bool raw) {
    check_3d(A, torch::kBFloat16, "A");
    check_3d(B, torch::kBFloat16, "B");
    ll E = A.size(0), L = A.size(1), VA = A.size(2), VB = B.size(2);
    TORCH_CHECK(B.size(0) == E && B.size(1) == L, "A/B epoch shapes differ");
    TORCH_CHECK(start >= 0 && start + count <= VA, "voxel range");
    TORCH_CHECK(P > 0 && E % P == 0, "epochs_per_subj must divide E");
    TORCH_CHECK(P <= 32, "epochs_per_subj > 32: use the staged path");
    TORCH_CHECK(fcma_corr_norm_smem(L, (int)P) <= 160 * 1024,
                "corr tile exceeds gfx950 LDS; use the staged path");
    TORCH_CHECK(fcma_supported_L(L) == L, kBadL);
    ll Eout = std::max((ll)padE, E);
    torch::Tensor Z;
    bool fp8 = false;
    if (out_opt.has_value()) {
        // caller-provided persistent buffer (rows >= E; padding rows
        // must be pre-zeroed once by the caller).  A Float8_e4m3fn
        // buffer selects the fp8 Z path (half the HBM round trip).
        Z = out_opt.value();
        fp8 = Z.scalar_type() == torch::kFloat8_e4m3fn;
        TORCH_CHECK(Z.is_cuda() && Z.is_contiguous()
                    && (fp8 || Z.scalar_type() == torch::kBFloat16)
                    && Z.size(0) >= count && Z.size(1) >= Eout
                    && Z.size(2) == VB, "bad out buffer");
        Eout = Z.size(1);
        if (Z.size(0) != count)
            Z = Z.narrow(0, 0, count);
    } else {
        Z = (Eout == E) ? torch::empty({count, E, VB}, A.options())
                        : torch::zeros({count, Eout, VB}, A.options());
    }
    // the dot3s kernel (P in {2,4}: every raw and fp8 launch, and the
    // bf16 corr+norm one) reads the A operand voxel-major through the
    // scalar path: hand it the [count, E, L] transposed slice
    torch::Tensor At;
    const void* At_ptr = nullptr;
    if (P == 2 || P == 4) {
        At = A.narrow(2, start, count).permute({2, 0, 1}).contiguous();
        At_ptr = At.data_ptr();
    }
    // the kernel writes rows [0, E) with row stride Eout directly
    if (raw) {
        TORCH_CHECK(!fp8, "raw correlations are bf16-only (e4m3 cannot "
                          "resolve r near +-1 before Fisher-z)");
        TORCH_CHECK(At_ptr != nullptr, "raw mode needs P in {2,4}");
        TORCH_CHECK(launch_fcma_corr_raw(At_ptr, B.data_ptr(),
                                         Z.data_ptr(), E, L, VB, count,
                                         Eout, (int)P, cur_stream()),
                    kNoKernel, "raw P=", P, " L=", L);
        return Z;
    }
    if (fp8) {
        TORCH_CHECK(fcma_corr_norm_z8_supported(E, (int)P, L),
                    "fp8 Z output needs P in {2,4} and even L");
        TORCH_CHECK(launch_fcma_corr_norm_z8(At_ptr, B.data_ptr(),
                                             Z.data_ptr(), E, L, VB,
                                             count, Eout, (int)P,
                                             cur_stream()),
                    kNoKernel, "fp8 P=", P, " L=", L);
        return Z;
    }
    TORCH_CHECK(launch_fcma_corr_norm(A.data_ptr(), B.data_ptr(),
                                      Z.data_ptr(), nullptr, E, L, VA, VB,
                                      start, count, (int)P, /*mode=*/0,
                                      Eout, cur_stream(), At_ptr),
                kNoKernel, "P=", P, " L=", L);
    return Z;
}

torch::Tensor fcma_gram_bf16(torch::Tensor Z, int64_t norm_P) {
    check_3d(Z, torch::kBFloat16, "Z");
    ll C = Z.size(0), E = Z.size(1), V = Z.size(2);
    TORCH_CHECK(E % 64 == 0, "E must be a multiple of 64 (host pads)");
    ll eb = E / 64;
    // V-split for latency hiding: PMC shows the kernel 84 % parked on
    // its serial k-tile loop at 4 blocks/CU — target ~8 blocks/CU
    ll base = C * eb * eb;
    ll ktAll = (V + 63) / 64;
    // measured sweep (profiles/README.md r2): ~8k blocks in flight
    // beats the old ~2k target by 0.3 ms/step; 16k regresses
    ll nsplit = std::min(ktAll, std::max((ll)1, (8191 + base) / base));
    if (const char* e = getenv("BRAINIAK_GRAM_NSPLIT"))
        nsplit = std::min(ktAll, std::max((ll)1, (ll)atoll(e)));
    TORCH_CHECK(norm_P == 0 || norm_P == 2 || norm_P == 4,
                "norm_P must be 0 (pre-normalized) or 2/4");
    if (norm_P)
        TORCH_CHECK(E % 64 == 0 && 64 % norm_P == 0,
                    "fused normalize needs band-aligned subjects");
    auto launch = [&](float* g, ll ns) {
        if (norm_P)
            launch_fcma_gram_bf16_norm(Z.data_ptr(), g, C, E, V, ns,
                                       (int)norm_P, cur_stream());
        else
            launch_fcma_gram_bf16(Z.data_ptr(), g, C, E, V, ns,
                                  cur_stream());
    };
    if (nsplit <= 1) {
        auto G = torch::empty({C, E, E},
                              Z.options().dtype(torch::kFloat32));
        launch(G.data_ptr<float>(), 1);
        return G;
    }
    auto Gp = torch::empty({nsplit, C, E, E},
                           Z.options().dtype(torch::kFloat32));
    launch(Gp.data_ptr<float>(), nsplit);
    return Gp.sum(0);
}

void fcma_corr_gram_duo(torch::Tensor A, torch::Tensor B,
                        int64_t start, int64_t count, int64_t P,
                        torch::Tensor Zout,
                        c10::optional<torch::Tensor> Zprev,
                        c10::optional<torch::Tensor> Gpart,
                        c10::optional<torch::Tensor> Gsum_part,
                        c10::optional<torch::Tensor> Gsum_out,
                        bool shrink) {
    // one grid = raw-corr blocks for [start, start+count) + Gram
    // (+in-register normalize) blocks for the PREVIOUS chunk's Z
    check_3d(A, torch::kBFloat16, "A");
    check_3d(B, torch::kBFloat16, "B");
    ll E = A.size(0), L = A.size(1), VA = A.size(2), VB = B.size(2);
    TORCH_CHECK(start >= 0 && start + count <= VA, "voxel range");
    TORCH_CHECK(P == 2 || P == 4, "duo path needs P in {2,4}");
    TORCH_CHECK(fcma_supported_L(L) == L, "L must be a supported "
                "template length");
    TORCH_CHECK(Zout.is_cuda() && Zout.is_contiguous()
                && Zout.scalar_type() == torch::kBFloat16
                && Zout.size(0) >= count && Zout.size(2) == VB,
                "bad Zout");
    ll Eout = Zout.size(1);
    auto At = A.narrow(2, start, count).permute({2, 0, 1}).contiguous();

    const void* zprev_ptr = nullptr;
    float* g_ptr = nullptr;
    ll Cg = 0, Eg = 0, Vg = 0, nsplit = 1;
    if (Gpart.has_value()) {
        TORCH_CHECK(Zprev.has_value(), "Gpart needs Zprev");
        auto& Zp = Zprev.value();
        auto& G = Gpart.value();
        TORCH_CHECK(Zp.is_cuda() && Zp.is_contiguous()
                    && Zp.scalar_type() == torch::kBFloat16, "bad Zprev");
        TORCH_CHECK(G.is_cuda() && G.is_contiguous() && G.dim() == 4
                    && G.scalar_type() == torch::kFloat32, "bad Gpart");
        Cg = G.size(1); Eg = Zp.size(1); Vg = Zp.size(2);
        nsplit = G.size(0);
        TORCH_CHECK(Eg % 64 == 0 && G.size(2) == Eg && G.size(3) == Eg,
                    "Gpart/Zprev shape mismatch");
        TORCH_CHECK(Zp.size(0) >= Cg, "Zprev rows < Cg");
        zprev_ptr = Zp.data_ptr();
        g_ptr = G.data_ptr<float>();
    }
    const float* gps_ptr = nullptr;
    float* gso_ptr = nullptr;
    ll Cs = 0, nsplit_sum = 1;
    if (Gsum_out.has_value()) {
        TORCH_CHECK(Gsum_part.has_value(), "Gsum_out needs Gsum_part");
        auto& Gp = Gsum_part.value();
        auto& Go = Gsum_out.value();
        TORCH_CHECK(Gp.is_cuda() && Gp.is_contiguous() && Gp.dim() == 4
                    && Gp.scalar_type() == torch::kFloat32,
                    "bad Gsum_part");
        TORCH_CHECK(Go.is_cuda() && Go.is_contiguous() && Go.dim() == 3
                    && Go.scalar_type() == torch::kFloat32,
                    "bad Gsum_out");
        Cs = Go.size(0);
        nsplit_sum = Gp.size(0);
        TORCH_CHECK(Gp.size(2) == Go.size(1)
                    && Gp.size(3) == Go.size(2)
                    && (Eg == 0 || Go.size(1) == Eg),
                    "Gsum shapes mismatch");
        // gsum_body strides by the partials' voxel-row count
        TORCH_CHECK(Gp.size(1) == Cs,
                    "Gsum_part rows must equal Gsum_out rows");
        gps_ptr = Gp.data_ptr<float>();
        gso_ptr = Go.data_ptr<float>();
    }
    TORCH_CHECK(launch_fcma_corr_gram_duo(
                    At.data_ptr(), B.data_ptr(), Zout.data_ptr(), E, L,
                    VB, count, Eout, (int)P, zprev_ptr, g_ptr, Cg, Eg,
                    Vg, nsplit, gps_ptr, gso_ptr, Cs, nsplit_sum,
                    shrink ? 1 : 0, cur_stream()),
                kNoKernel, "duo P=", P, " L=", L);
}

torch::Tensor debug_fp8_cvt(torch::Tensor x, bool sw) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kFloat32);
    auto xc = x.contiguous();
    auto o = torch::empty_like(xc, xc.options()
                                       .dtype(torch::kFloat8_e4m3fn));
    if (sw)
        launch_fp8_cvt_probe_sw(xc.data_ptr<float>(), o.data_ptr(),
                                xc.numel(), cur_stream());
    else
        launch_fp8_cvt_probe(xc.data_ptr<float>(), o.data_ptr(),
                             xc.numel(), cur_stream());
    return o;
}

torch::Tensor fcma_gram_fp8(torch::Tensor Z) {
    TORCH_CHECK(Z.is_cuda() && Z.dim() == 3 && Z.is_contiguous()
                && Z.scalar_type() == torch::kFloat8_e4m3fn,
                "Z must be contiguous [C,E,V] float8_e4m3fn on GPU");
    ll C = Z.size(0), E = Z.size(1), V = Z.size(2);
    TORCH_CHECK(E % 64 == 0, "E must be a multiple of 64 (host pads)");
    TORCH_CHECK(V % 16 == 0, "V must be a multiple of 16 (host pads)");
    ll eb = E / 64;
    ll base = C * eb * eb;
    ll ktAll = (V + 255) / 256;
    ll nsplit = std::min(ktAll, std::max((ll)1, (2047 + base) / base));
    if (nsplit <= 1) {
        auto G = torch::empty({C, E, E},
                              Z.options().dtype(torch::kFloat32));
        launch_fcma_gram_fp8(Z.data_ptr(), G.data_ptr<float>(), C, E, V,
                             1, cur_stream());
        return G;
    }
    auto Gp = torch::empty({nsplit, C, E, E},
                           Z.options().dtype(torch::kFloat32));
    launch_fcma_gram_fp8(Z.data_ptr(), Gp.data_ptr<float>(), C, E, V,
                         nsplit, cur_stream());
    return Gp.sum(0);
}

torch::Tensor fcma_gram(torch::Tensor corr) {
    check_3d(corr, torch::kFloat32, "corr");
    ll C = corr.size(0), E = corr.size(1), V = corr.size(2);
    ll Epad = ((E + 63) / 64) * 64;
    torch::Tensor in = corr;
    if (Epad != E) {
        in = torch::zeros({C, Epad, V}, corr.options());
        in.narrow(1, 0, E).copy_(corr);
    }
    auto G = torch::empty({C, Epad, Epad},
                          corr.options().dtype(torch::kFloat32));
    launch_fcma_gram_f32(in.data_ptr<float>(), G.data_ptr<float>(), C,
                         Epad, V, cur_stream());
    if (Epad != E)
        return G.narrow(1, 0, E).narrow(2, 0, E).contiguous();
    return G;
}

torch::Tensor fcma_fused_gram(torch::Tensor A, torch::Tensor B,
                              int64_t start, int64_t count, int64_t P) {
    ll E = A.size(0), L = A.size(1), VA = A.size(2), VB = B.size(2);
    if (fcma_fused_gram_supported(E, (int)P, L)) {
        // single-kernel path: Z never leaves LDS (see
        // fcma_kernels.hip::k_fused_corr_gram)
        check_3d(A, torch::kBFloat16, "A");
        check_3d(B, torch::kBFloat16, "B");
        TORCH_CHECK(B.size(0) == E && B.size(1) == L,
                    "A/B epoch shapes differ");
        TORCH_CHECK(start >= 0 && start + count <= VA, "voxel range");
        ll cTiles = (count + 7) / 8;
        ll vTiles = std::max((ll)1, (VB + 63) / 64);
        // enough workgroups to fill 256 CUs (1 resident WG per CU),
        // but never more v-splits than v-windows
        int nsplit = (int)std::min(
            vTiles, std::max((ll)1, (511 + cTiles) / cTiles));
        auto G = torch::empty({nsplit, count, E, E},
                              A.options().dtype(torch::kFloat32));
        TORCH_CHECK(launch_fcma_fused_corr_gram(
                        A.data_ptr(), B.data_ptr(), G.data_ptr<float>(),
                        L, VA, VB, start, count, nsplit, cur_stream()),
                    kNoKernel, "fused L=", L);
        return nsplit == 1 ? G.squeeze(0) : G.sum(0);
    }
    ll Epad = ((E + 63) / 64) * 64;
    auto Z = fcma_corr_norm_z(A, B, start, count, P, Epad, c10::nullopt,
                              /*raw=*/false);
    auto G = fcma_gram_bf16(Z, /*norm_P=*/0);
    if (Epad != E)
        return G.narrow(1, 0, E).narrow(2, 0, E).contiguous();
    return G;
}

// Single-kernel correlation + normalize + Gram over the cached
// time-contiguous operands (fcma_fused_kernels.hip).  At_all / B_t are
// [64, V, LP] bf16: epoch rows past E and time steps past L zero-filled.
// Returns [count, 64, 64] fp32, shrunk when asked; nsplit > 1 cuts the
// column sweep into ranges whose partials gsum reduces in fixed order.
// clamp = "auto" clamps the Fisher z only in tasks that hold an |r| >= 1;
// "always" clamps every element (same bits for finite operands).
// schedule = "ahead" issues each task's correlation MFMAs one task before
// its normalize (column prefetch two tasks deep), "phased" at the head of
// the task itself (the order the kernel was first shipped with); "auto"
// is "ahead".  The LP = 64 instances have no "ahead" form and run phased
// either way.  All give the same bits.
// fisher = "table" takes the Fisher z of the unclamped normalize from a
// table of the bf16 magnitudes that every workgroup builds in LDS,
// "log" computes it (v_log_f32); "auto" is the table where the instance
// has one (fcma_corr_gram_fused_table) and clamp is "auto".  Asking for
// the table where there is none is an error.  Both give the same bits.
// partials = true returns the [nsplit, count, 64, 64] slabs as the kernel
// wrote them (unshrunk, not summed); a split without a column window
// is an all-zero slab.
static torch::Tensor fcma_corr_gram_fused_impl(
    torch::Tensor At_all, torch::Tensor B_t, int64_t start, int64_t count,
    int64_t P, int64_t nsplit, bool shrink, const std::string& clamp,
    const std::string& schedule, const std::string& fisher,
    bool partials) {
    check_3d(At_all, torch::kBFloat16, "At_all");
    check_3d(B_t, torch::kBFloat16, "B_t");
    ll VA = At_all.size(1), VB = B_t.size(1), LP = At_all.size(2);
    TORCH_CHECK(At_all.size(0) == 64 && B_t.size(0) == 64,
                "fused operands carry 64 (zero-padded) epoch rows");
    TORCH_CHECK(B_t.size(2) == LP && (LP == 16 || LP == 32 || LP == 64),
                "fused operand row length must be 16, 32 or 64");
    TORCH_CHECK(VB >= 16 && VB % 16 == 0,
                "data2 voxel count must be a multiple of 16 (host pads)");
    TORCH_CHECK(P == 2 || P == 4, "fused path needs P in {2,4}");
    // the kernel keeps per-lane row offsets in 32 bits
    TORCH_CHECK(VA * LP < (1LL << 31) && VB * LP < (1LL << 31),
                "voxel count too large for the fused kernel");
    TORCH_CHECK(start >= 0 && count > 0 && start + count <= VA,
                "voxel range");
    ll windows = (VB + fcma_corr_gram_fused_vt() - 1)
        / fcma_corr_gram_fused_vt();
    // The Gram entry point takes at most one split per window.  The slab
    // view takes up to twice that: it exists to show splits without a
    // window (all-zero slabs), and with few windows those only arise
    // past that limit (two windows cut three ways).
    if (partials) {
        TORCH_CHECK(nsplit >= 1 && nsplit <= 2 * windows,
                    "nsplit must be in [1, 2 x column windows] for the "
                    "slab view");
    } else {
        TORCH_CHECK(nsplit >= 1 && nsplit <= windows,
                    "nsplit must be in [1, column windows]");
    }
    TORCH_CHECK(clamp == "auto" || clamp == "always",
                "clamp must be \"auto\" or \"always\"");
    const int force_clamp = clamp == "always" ? 1 : 0;
    TORCH_CHECK(schedule == "auto" || schedule == "ahead"
                || schedule == "phased",
                "schedule must be \"auto\", \"ahead\" or \"phased\"");
    // FS_SCHED_* of fcma_fused_kernels.hip
    const int sched = schedule == "auto" ? 0
        : (schedule == "ahead" ? 1 : 2);
    TORCH_CHECK(fisher == "auto" || fisher == "table" || fisher == "log",
                "fisher must be \"auto\", \"table\" or \"log\"");
    // FS_FISHER_* of fcma_fused_kernels.hip
    const int fish = fisher == "auto" ? 0 : (fisher == "table" ? 1 : 2);
    if (fish == 1) {
        TORCH_CHECK(!force_clamp, "fisher=\"table\" needs clamp=\"auto\": "
                    "the clamp=\"always\" instances keep the logs");
        TORCH_CHECK(fcma_corr_gram_fused_table((int)P, LP), kNoKernel,
                    "fused table instance for row length ", LP);
    }
    auto opts = At_all.options().dtype(torch::kFloat32);
    if (partials) {
        auto Gp = torch::empty({nsplit, count, 64, 64}, opts);
        launch_fcma_corr_gram_fused(At_all.data_ptr(), B_t.data_ptr(),
                                    Gp.data_ptr<float>(), (int)LP, VA, VB,
                                    start, count, (int)P, (int)nsplit, 0,
                                    force_clamp, sched, fish, cur_stream());
        return Gp;
    }
    auto G = torch::empty({count, 64, 64}, opts);
    if (nsplit == 1) {
        launch_fcma_corr_gram_fused(At_all.data_ptr(), B_t.data_ptr(),
                                    G.data_ptr<float>(), (int)LP, VA, VB,
                                    start, count, (int)P, 1,
                                    shrink ? 1 : 0, force_clamp, sched,
                                    fish, cur_stream());
        return G;
    }
    auto Gp = torch::empty({nsplit, count, 64, 64}, opts);
    launch_fcma_corr_gram_fused(At_all.data_ptr(), B_t.data_ptr(),
                                Gp.data_ptr<float>(), (int)LP, VA, VB,
                                start, count, (int)P, (int)nsplit, 0,
                                force_clamp, sched, fish, cur_stream());
    launch_fcma_gsum(Gp.data_ptr<float>(), G.data_ptr<float>(), count,
                     64 * 64, nsplit, shrink ? 1 : 0, cur_stream());
    return G;
}

torch::Tensor fcma_corr_gram_fused(torch::Tensor At_all, torch::Tensor B_t,
                                   int64_t start, int64_t count, int64_t P,
                                   int64_t nsplit, bool shrink,
                                   const std::string& clamp,
                                   const std::string& schedule,
                                   const std::string& fisher) {
    return fcma_corr_gram_fused_impl(At_all, B_t, start, count, P, nsplit,
                                     shrink, clamp, schedule, fisher, false);
}

torch::Tensor fcma_corr_gram_fused_partials(
    torch::Tensor At_all, torch::Tensor B_t, int64_t start, int64_t count,
    int64_t P, int64_t nsplit, const std::string& clamp,
    const std::string& schedule, const std::string& fisher) {
    return fcma_corr_gram_fused_impl(At_all, B_t, start, count, P, nsplit,
                                     false, clamp, schedule, fisher, true);
}

// Tests only.  r: fp32 values (bf16 patterns widened).  Returns the table
// as a workgroup builds it, the z of the log path and the z of the
// lookup for every r ([2, n]: r in the low and in the high half of a
// bf16 pair), from the device functions the fused kernel runs.
std::vector<torch::Tensor> fcma_fisher_table_probe(torch::Tensor r) {
    TORCH_CHECK(r.is_cuda() && r.dtype() == torch::kFloat32 && r.dim() == 1
                && r.is_contiguous(), "r: contiguous 1-D fp32 on the device");
    auto tab = torch::empty({fcma_fisher_table_entries()}, r.options());
    auto zlog = torch::empty_like(r);
    auto ztab = torch::empty({2, r.numel()}, r.options());
    launch_fcma_fisher_table_probe(r.data_ptr<float>(), r.numel(),
                                   tab.data_ptr<float>(),
                                   zlog.data_ptr<float>(),
                                   ztab.data_ptr<float>(), cur_stream());
    return {tab, zlog, ztab};
}

// Tests only.  The layout of the fused kernel's z image in LDS from the
// address functions the kernel runs, evaluated on the host: (stride,
// image bytes, LDS bytes ahead of the first image in the table instances,
// store offsets int32 [8, 64/P/8, 2, P, 64] by (wave, si, st, p, lane),
// read offsets int32 [16, 4, 64] by (voxel, band, lane)).
std::tuple<int64_t, int64_t, int64_t, torch::Tensor, torch::Tensor>
fcma_fused_image_layout_py(int64_t P) {
    TORCH_CHECK(P == 2 || P == 4, "fused path needs P in {2,4}");
    auto store = torch::empty({8, 64 / P / 8, 2, P, 64}, torch::kInt32);
    auto read = torch::empty({16, 4, 64}, torch::kInt32);
    int dims[3];
    fcma_fused_image_layout((int)P, dims, store.data_ptr<int>(),
                            read.data_ptr<int>());
    return {dims[0], dims[1], dims[2], store, read};
}

bool fcma_fused_gram_native(int64_t E, int64_t P, int64_t L) {
    return fcma_fused_gram_supported(E, (int)P, L) != 0;
}

// ---------------------------------------------------------------------------

std::vector<torch::Tensor> jacobi_eigh(torch::Tensor G) {
    check_3d(G, torch::kFloat32, "G");
    ll B = G.size(0);
    int K = (int)G.size(1);
    TORCH_CHECK(G.size(2) == K && K <= 64, "G must be [B,K,K], K<=64");
    auto evecs = torch::empty_like(G);
    auto evals = torch::empty({B, K}, G.options());
    launch_jacobi_eigh(G.data_ptr<float>(), evecs.data_ptr<float>(),
                       evals.data_ptr<float>(), B, K, cur_stream());
    return {evals, evecs};
}

torch::Tensor polar_invsqrt(torch::Tensor G) {
    // G^{-1/2} for a stack of SPD K x K Gram matrices via the batched
    // one-workgroup Jacobi eigensolver.  Lets callers with RAGGED
    // [V_i, K] factors (SRM subjects of different voxel counts) batch
    // the eigensolve while keeping per-subject GEMMs.
    TORCH_CHECK(G.is_cuda() && G.dim() == 3 && G.size(1) == G.size(2),
                "G must be [B,K,K] on GPU");
    TORCH_CHECK(G.size(1) <= 64, "K must be <= 64");
    auto Gf = G.to(torch::kFloat32).contiguous();
    auto ev = jacobi_eigh(Gf);
    auto lam = ev[0].clamp_min(1e-30);
    auto Vc = ev[1];
    return torch::bmm(Vc * lam.rsqrt().unsqueeze(1),
                      Vc.transpose(1, 2));
}

torch::Tensor batched_polar(torch::Tensor A, double perturb) {
    TORCH_CHECK(A.is_cuda() && A.dim() == 3, "A must be [B,V,K] on GPU");
    auto Af = A.to(torch::kFloat32).contiguous();
    ll K = Af.size(2);
    TORCH_CHECK(K <= 64, "K must be <= 64");
    if (perturb != 0.0) {
        Af = Af.clone();
        ll d = std::min(Af.size(1), Af.size(2));
        auto idx = torch::arange(d, torch::TensorOptions()
                                        .dtype(torch::kLong)
                                        .device(Af.device()));
        auto diag = Af.index({torch::indexing::Slice(), idx, idx});
        Af.index_put_({torch::indexing::Slice(), idx, idx},
                      diag + perturb);
    }
    auto G = torch::bmm(Af.transpose(1, 2), Af).contiguous();  // [B,K,K]
    // W = A G^{-1/2}
    return torch::bmm(Af, polar_invsqrt(G));
}

// ---------------------------------------------------------------------------

torch::Tensor tfa_factor(torch::Tensor centers, torch::Tensor widths,
                         torch::Tensor coords) {
    TORCH_CHECK(centers.is_cuda() && centers.dim() == 2 &&
                centers.size(1) == 3, "centers must be [K,3] on GPU");
    TORCH_CHECK(coords.dim() == 2 && coords.size(1) == 3,
                "coords must be [V,3]");
    auto c = centers.to(torch::kFloat32).contiguous();
    auto w = widths.to(torch::kFloat32).contiguous();
    auto x = coords.to(torch::kFloat32).contiguous();
    int K = (int)c.size(0);
    ll V = x.size(0);
    TORCH_CHECK(K <= 128, "K must be <= 128");
    auto F = torch::empty({V, K}, c.options());
    launch_tfa_factor(c.data_ptr<float>(), w.data_ptr<float>(),
                      x.data_ptr<float>(), F.data_ptr<float>(), V, K,
                      cur_stream());
    return F;
}

torch::Tensor tfa_recon(torch::Tensor X, torch::Tensor W, torch::Tensor F,
                        double scale) {
    TORCH_CHECK(X.is_cuda() && X.dim() == 2, "X must be [V,T] on GPU");
    auto Xf = X.to(torch::kFloat32).contiguous();
    auto Wf = W.to(torch::kFloat32).contiguous();
    auto Ff = F.to(torch::kFloat32).contiguous();
    ll V = Xf.size(0), T = Xf.size(1);
    int K = (int)Wf.size(0);
    TORCH_CHECK(Ff.size(0) == V && Ff.size(1) == K && Wf.size(1) == T,
                "shape mismatch");
    auto R = torch::empty({V * T}, Xf.options());
    launch_tfa_recon(Xf.data_ptr<float>(), Wf.data_ptr<float>(),
                     Ff.data_ptr<float>(), R.data_ptr<float>(), V, T, K,
                     (float)scale, cur_stream());
    return R;
}

// trace: also return the decision values [C,F,E] and iteration counts
// [C,F] of the TRACE kernel instantiations (svm_cv_trace, tests only)
static std::vector<torch::Tensor> svm_cv_impl(
        torch::Tensor kernels, torch::Tensor y, torch::Tensor train_idx,
        torch::Tensor test_idx, torch::Tensor n_train, torch::Tensor n_test,
        double Creg, double tol, int64_t max_iter, int64_t max_n_hint,
        const std::string& variant, bool trace) {
    check_3d(kernels, torch::kFloat32, "kernels");
    ll C = kernels.size(0);
    int E = (int)kernels.size(1);
    TORCH_CHECK(kernels.size(2) == E, "kernels must be [C,E,E]");
    int F = (int)train_idx.size(0);
    TORCH_CHECK(y.is_cuda() && y.scalar_type() == torch::kFloat32 &&
                y.numel() == E, "y must be fp32 [E] on GPU");
    TORCH_CHECK(train_idx.scalar_type() == torch::kInt32 &&
                test_idx.scalar_type() == torch::kInt32, "idx int32");
    TORCH_CHECK(train_idx.size(1) == E && test_idx.size(1) == E,
                "idx must be [F,E]");
    auto nt = n_train.to(torch::kInt32).contiguous();
    auto ns = n_test.to(torch::kInt32).contiguous();
    // max_n_hint lets the caller skip the .item() device sync (needed
    // when this launch is enqueued on a side stream mid-pipeline)
    ll max_n = max_n_hint > 0
        ? max_n_hint
        : std::max<ll>(nt.max().item<int>(), ns.max().item<int>());
    TORCH_CHECK(max_n <= 128,
                "svm_cv supports fold sizes up to 128 samples");
    // "shared": one workgroup per voxel, the folds share one K tile;
    // "wave": one wave per (voxel, fold) QP; "auto": shared when its
    // tile fits.  Both give the same counts.
    TORCH_CHECK(variant == "auto" || variant == "shared" ||
                variant == "wave",
                "variant must be \"auto\", \"shared\" or \"wave\"");
    TORCH_CHECK(variant != "shared" || svm_cv_shared_fits(E, max_n),
                "svm_cv variant \"shared\" needs E <= 128 and an [E,E] "
                "tile within 64 KB of LDS; got E=", E, ", fold size ",
                max_n);
    const int variant_id = variant == "shared" ? 1
                         : variant == "wave" ? 2 : 0;
    auto correct = torch::zeros({C, F}, kernels.options()
                                            .dtype(torch::kInt32));
    if (!trace) {
        launch_svm_cv(kernels.data_ptr<float>(), y.data_ptr<float>(),
                      train_idx.data_ptr<int>(), test_idx.data_ptr<int>(),
                      nt.data_ptr<int>(), ns.data_ptr<int>(),
                      correct.data_ptr<int>(), C, E, F, (float)Creg,
                      (float)tol, (int)max_iter, max_n, variant_id,
                      cur_stream());
        return {correct};
    }
    auto dec = torch::zeros({C, F, E}, kernels.options());
    auto n_iter = torch::zeros({C, F}, correct.options());
    launch_svm_cv_trace(kernels.data_ptr<float>(), y.data_ptr<float>(),
                        train_idx.data_ptr<int>(), test_idx.data_ptr<int>(),
                        nt.data_ptr<int>(), ns.data_ptr<int>(),
                        correct.data_ptr<int>(), dec.data_ptr<float>(),
                        n_iter.data_ptr<int>(), C, E, F, (float)Creg,
                        (float)tol, (int)max_iter, max_n, variant_id,
                        cur_stream());
    return {correct, dec, n_iter};
}

torch::Tensor svm_cv(torch::Tensor kernels, torch::Tensor y,
                     torch::Tensor train_idx, torch::Tensor test_idx,
                     torch::Tensor n_train, torch::Tensor n_test,
                     double Creg, double tol, int64_t max_iter,
                     int64_t max_n_hint, const std::string& variant) {
    return svm_cv_impl(kernels, y, train_idx, test_idx, n_train, n_test,
                       Creg, tol, max_iter, max_n_hint, variant, false)[0];
}

std::vector<torch::Tensor> svm_cv_trace(
        torch::Tensor kernels, torch::Tensor y, torch::Tensor train_idx,
        torch::Tensor test_idx, torch::Tensor n_train, torch::Tensor n_test,
        double Creg, double tol, int64_t max_iter, int64_t max_n_hint,
        const std::string& variant) {
    return svm_cv_impl(kernels, y, train_idx, test_idx, n_train, n_test,
                       Creg, tol, max_iter, max_n_hint, variant, true);
}

torch::Tensor stencil3d(torch::Tensor x, torch::Tensor w) {
    TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.is_contiguous()
                && w.is_contiguous()
                && x.scalar_type() == torch::kFloat32
                && w.scalar_type() == torch::kFloat32
                && x.dim() == 4 && w.dim() == 3,
                "x must be [B,X,Y,Z] fp32, w [K,K,K] fp32 on GPU");
    ll K = w.size(0);
    TORCH_CHECK(w.size(1) == K && w.size(2) == K && K % 2 == 1 && K <= 9,
                "w must be cubic with odd K <= 9");
    int r = (int)(K / 2);
    ll B = x.size(0);
    int X = (int)x.size(1), Y = (int)x.size(2), Z = (int)x.size(3);
    TORCH_CHECK(X > 2 * r && Y > 2 * r && Z > 2 * r,
                "volume smaller than the kernel");
    auto out = torch::empty({B, X - 2 * r, Y - 2 * r, Z - 2 * r},
                            x.options());
    launch_stencil3d(x.data_ptr<float>(), w.data_ptr<float>(),
                     out.data_ptr<float>(), B, X, Y, Z, r,
                     cur_stream());
    return out;
}

torch::Tensor isfc_fused_(torch::Tensor acc, torch::Tensor Zs,
                          torch::Tensor Zm) {
    TORCH_CHECK(acc.is_cuda() && acc.is_contiguous() && acc.dim() == 2
                && acc.scalar_type() == torch::kFloat32
                && acc.size(0) == acc.size(1), "acc must be fp32 [V,V]");
    for (auto* Z : {&Zs, &Zm}) {
        TORCH_CHECK(Z->is_cuda() && Z->is_contiguous()
                    && Z->dim() == 3
                    && Z->scalar_type() == torch::kBFloat16,
                    "Z stacks must be bf16 [B,V,T]");
    }
    TORCH_CHECK(Zs.sizes() == Zm.sizes(), "Zs/Zm shape mismatch");
    TORCH_CHECK(Zs.size(1) == acc.size(0), "V mismatch");
    launch_isfc_fused(acc.data_ptr<float>(), Zs.data_ptr(),
                      Zm.data_ptr(), Zs.size(1), Zs.size(2),
                      Zs.size(0), cur_stream());
    return acc;
}

torch::Tensor isfc_accum_(torch::Tensor acc, torch::Tensor M) {
    // M: [V, V] or a [B, V, V] subject stack (the batch amortizes the
    // acc read-modify-write across B matrices in one pass)
    bool m_bf16 = M.scalar_type() == torch::kBFloat16;
    ll B = (M.dim() == 3) ? M.size(0) : 1;
    ll V = acc.size(0);
    TORCH_CHECK(acc.is_cuda() && M.is_cuda() && acc.is_contiguous()
                && M.is_contiguous()
                && acc.scalar_type() == torch::kFloat32
                && (m_bf16 || M.scalar_type() == torch::kFloat32)
                && acc.dim() == 2 && acc.size(1) == V
                && (M.dim() == 2 || M.dim() == 3)
                && M.size(-1) == V && M.size(-2) == V,
                "acc fp32 [V,V] / M fp32-or-bf16 [V,V] or [B,V,V]");
    launch_isfc_accum(acc.data_ptr<float>(), M.data_ptr(),
                      V, B, m_bf16 ? 1 : 0, cur_stream());
    return acc;
}

// argument checks shared by the two chain-graph recursions
static void check_hmm_args(const char* op, const torch::Tensor& logprob,
                           const torch::Tensor& log_start,
                           const torch::Tensor& log_end,
                           const torch::Tensor& log_self,
                           const torch::Tensor& log_adv,
                           const torch::Tensor& pred,
                           const torch::Tensor& succ) {
    check_3d(logprob, torch::kFloat64, "logprob");
    ll B = logprob.size(0), T = logprob.size(1), K = logprob.size(2);
    TORCH_CHECK(K >= 1 && K <= 64, op, " needs "
                "1 <= K <= 64 event states (got ", K, ")");
    TORCH_CHECK(T >= 1 && T <= INT_MAX / 64, "T out of range");
    TORCH_CHECK(B <= INT_MAX, "too many sequences for one launch");
    for (auto* v : {&log_start, &log_end, &log_self, &log_adv}) {
        TORCH_CHECK(v->is_cuda() && v->is_contiguous() && v->dim() == 1
                    && v->scalar_type() == torch::kFloat64
                    && v->device() == logprob.device(),
                    "chain vectors must be contiguous fp64 [>=K] on GPU");
    }
    // log_start / log_end may carry the sink entry after the K events
    TORCH_CHECK(log_start.size(0) >= K && log_end.size(0) >= K,
                "log_start/log_end must have at least K entries");
    TORCH_CHECK(log_self.size(0) == K && log_adv.size(0) == K,
                "log_self/log_adv must have K entries");
    for (auto* v : {&pred, &succ}) {
        TORCH_CHECK(v->is_cuda() && v->is_contiguous() && v->dim() == 1
                    && v->scalar_type() == torch::kInt32
                    && v->size(0) == K
                    && v->device() == logprob.device(),
                    "pred/succ must be contiguous int32 [K] on GPU");
    }
}

std::vector<torch::Tensor> hmm_forward_backward(
        torch::Tensor logprob, torch::Tensor log_start,
        torch::Tensor log_end, torch::Tensor log_self,
        torch::Tensor log_adv, torch::Tensor pred, torch::Tensor succ) {
    // single-launch log-space forward-backward over the K event states
    // of EventSegment's chain graph (hmm_kernels.hip::k_hmm_fb)
    check_hmm_args("hmm_forward_backward", logprob, log_start, log_end,
                   log_self, log_adv, pred, succ);
    ll B = logprob.size(0), T = logprob.size(1), K = logprob.size(2);
    auto log_gamma = torch::empty({B, T, K}, logprob.options());
    auto llik = torch::empty({B}, logprob.options());
    if (B == 0) return {log_gamma, llik};
    launch_hmm_fb(logprob.data_ptr<double>(), log_start.data_ptr<double>(),
                  log_end.data_ptr<double>(), log_self.data_ptr<double>(),
                  log_adv.data_ptr<double>(), pred.data_ptr<int>(),
                  succ.data_ptr<int>(), log_gamma.data_ptr<double>(),
                  llik.data_ptr<double>(), B, (int)T, (int)K,
                  cur_stream());
    return {log_gamma, llik};
}

std::vector<torch::Tensor> hmm_viterbi(
        torch::Tensor logprob, torch::Tensor log_start,
        torch::Tensor log_end, torch::Tensor log_self,
        torch::Tensor log_adv, torch::Tensor pred, torch::Tensor succ) {
    // single-launch MAP path over the same chain graph
    // (hmm_kernels.hip::k_hmm_viterbi); succ is checked for interface
    // symmetry, the recursion only walks pred
    check_hmm_args("hmm_viterbi", logprob, log_start, log_end, log_self,
                   log_adv, pred, succ);
    ll B = logprob.size(0), T = logprob.size(1), K = logprob.size(2);
    auto path = torch::empty({B, T}, logprob.options().dtype(torch::kInt32));
    auto score = torch::empty({B}, logprob.options());
    if (B == 0) return {path, score};
    // one 64-bit back-pointer word per (sequence, timestep)
    auto masks = torch::empty({B, T},
                              logprob.options().dtype(torch::kInt64));
    launch_hmm_viterbi(logprob.data_ptr<double>(),
                       log_start.data_ptr<double>(),
                       log_end.data_ptr<double>(),
                       log_self.data_ptr<double>(),
                       log_adv.data_ptr<double>(), pred.data_ptr<int>(),
                       (ll*)masks.data_ptr<int64_t>(), path.data_ptr<int>(),
                       score.data_ptr<double>(), B, (int)T, (int)K,
                       cur_stream());
    return {path, score};
}

// argument checks of the ISC resampling gather (index ranges are the
// Python caller's job: the indices are born on the host)
static void check_isc_resample_args(const torch::Tensor& table,
                                    const torch::Tensor& rows,
                                    const c10::optional<torch::Tensor>& lags,
                                    const torch::Tensor& signs,
                                    bool median) {
    check_3d(table, torch::kFloat64, "table");
    TORCH_CHECK(rows.is_cuda() && rows.is_contiguous() && rows.dim() == 2
                && rows.scalar_type() == torch::kInt32
                && rows.device() == table.device(),
                "rows must be contiguous int32 [I,R] on the table's GPU");
    TORCH_CHECK(signs.is_cuda() && signs.is_contiguous()
                && signs.scalar_type() == torch::kInt8
                && signs.device() == table.device()
                && signs.sizes() == rows.sizes(),
                "signs must be contiguous int8 [I,R] on the table's GPU");
    if (lags.has_value()) {
        const auto& lg = lags.value();
        TORCH_CHECK(lg.is_cuda() && lg.is_contiguous()
                    && lg.scalar_type() == torch::kInt32
                    && lg.device() == table.device()
                    && lg.sizes() == rows.sizes(),
                    "lags must be contiguous int32 [I,R] on the table's "
                    "GPU (or None)");
    }
    ll I = rows.size(0), R = rows.size(1), V = table.size(2);
    TORCH_CHECK(R <= INT_MAX, "too many rows per draw");
    TORCH_CHECK(!median || R <= isc_resample_max_rows(),
                "isc_resample_stat 'median' needs R <= ",
                isc_resample_max_rows(), " rows per draw (got ", R, ")");
    TORCH_CHECK(R == 0 || (table.size(0) >= 1 && table.size(1) >= 1),
                "table has no rows to gather from");
    TORCH_CHECK(I * ((V + 63) / 64) <= (ll)INT_MAX,
                "too many (draw, voxel tile) blocks for one launch");
}

torch::Tensor isc_resample_stat(torch::Tensor table, torch::Tensor rows,
                                c10::optional<torch::Tensor> lags,
                                torch::Tensor signs, std::string stat) {
    // per-draw gather + nan-skipping median / Fisher mean
    // (isc_stats_kernels.hip::k_isc_resample_stat)
    TORCH_CHECK(stat == "median" || stat == "mean",
                "stat must be 'median' or 'mean'");
    const bool median = stat == "median";
    check_isc_resample_args(table, rows, lags, signs, median);
    ll I = rows.size(0), R = rows.size(1);
    ll L = table.size(1), V = table.size(2);
    auto out = torch::empty({I, V}, table.options());
    if (I == 0 || V == 0) return out;
    launch_isc_resample_stat(
        table.data_ptr<double>(), rows.data_ptr<int>(),
        lags.has_value() ? lags.value().data_ptr<int>() : nullptr,
        (const signed char*)signs.data_ptr<int8_t>(),
        out.data_ptr<double>(), I, L, V, (int)R, median ? 1 : 0,
        cur_stream());
    return out;
}

torch::Tensor isc_phase_stat(torch::Tensor table, torch::Tensor coef,
                             std::string stat) {
    // x[i,r,v] = sum_k coef[i,r,k] * table[r,k,v], then the nan-skipping
    // median / Fisher mean over r (isc_stats_kernels.hip::k_isc_phase_stat)
    TORCH_CHECK(stat == "median" || stat == "mean",
                "stat must be 'median' or 'mean'");
    const bool median = stat == "median";
    check_3d(table, torch::kFloat64, "table");
    TORCH_CHECK(coef.is_cuda() && coef.is_contiguous() && coef.dim() == 3
                && coef.scalar_type() == torch::kFloat64
                && coef.device() == table.device(),
                "coef must be contiguous fp64 [I,R,K] on the table's GPU");
    ll R = table.size(0), K = table.size(1), V = table.size(2);
    ll I = coef.size(0);
    TORCH_CHECK(coef.size(1) == R && coef.size(2) == K,
                "coef [I,R,K] must agree with table [R,K,V] in R and K");
    TORCH_CHECK(R >= 1 && K >= 1, "table needs at least one row and one "
                "column");
    TORCH_CHECK(!median || R <= isc_phase_max_rows(),
                "isc_phase_stat 'median' needs R <= ", isc_phase_max_rows(),
                " rows (got ", R, ")");
    // segment and voxel indices are 32-bit factors of a 64-bit offset
    TORCH_CHECK(R * K <= (ll)INT_MAX / 2, "too many table segments (R * K)");
    TORCH_CHECK(V <= (ll)INT_MAX, "too many voxels for one launch");
    auto out = torch::empty({I, V}, table.options());
    if (I == 0 || V == 0) return out;
    TORCH_CHECK(isc_phase_blocks(I, V, (int)R, median ? 1 : 0)
                    <= (ll)INT_MAX,
                "too many (voxel tile, draw tile) blocks for one launch");
    launch_isc_phase_stat(table.data_ptr<double>(), coef.data_ptr<double>(),
                          out.data_ptr<double>(), I, V, (int)R, (int)K,
                          median ? 1 : 0, cur_stream());
    return out;
}

// shared argument checks of the observed-ISC kernels: data fp64 [T,V,S]
// contiguous on the GPU, the voxel window [v0, v0 + nv) inside it
static void check_isc_corr_args(const torch::Tensor& data, ll v0, ll nv) {
    check_3d(data, torch::kFloat64, "data");
    ll T = data.size(0), V = data.size(1), S = data.size(2);
    TORCH_CHECK(T >= 1, "data needs at least one time point");
    TORCH_CHECK(S >= 2, "data needs at least two subjects (got ", S, ")");
    TORCH_CHECK(S <= (ll)INT_MAX / 4, "too many subjects");
    TORCH_CHECK(v0 >= 0 && nv >= 0 && v0 <= V && nv <= V - v0,
                "voxel window [", v0, ", ", v0 + nv, ") outside [0, ", V,
                ")");
}

torch::Tensor isc_loo(torch::Tensor data, bool tolerant, double min_clean,
                      ll v0, ll nv) {
    // leave-one-out ISC of the voxel window -> r [S, nv]
    // (isc_corr_kernels.hip::k_isc_totals, k_isc_loo, k_isc_drop)
    if (nv < 0) nv = data.dim() == 3 ? data.size(1) - v0 : 0;
    check_isc_corr_args(data, v0, nv);
    ll T = data.size(0), V = data.size(1), S = data.size(2);
    auto r = torch::empty({S, nv}, data.options());
    if (nv == 0) return r;
    TORCH_CHECK(isc_loo_blocks(T, nv, (int)S) <= (ll)INT_MAX,
                "too many blocks for one launch");
    auto tot = torch::empty({T, nv}, data.options());
    auto cnt = torch::empty({tolerant ? T : 0, nv},
                            data.options().dtype(torch::kInt32));
    auto flags = torch::empty({nv, S}, data.options().dtype(torch::kUInt8));
    launch_isc_loo(data.data_ptr<double>() + v0 * S, tot.data_ptr<double>(),
                   tolerant ? cnt.data_ptr<int>() : nullptr,
                   r.data_ptr<double>(), flags.data_ptr<uint8_t>(), V * S, T,
                   nv, (int)S, tolerant ? 1 : 0, min_clean, cur_stream());
    return r;
}

torch::Tensor isc_pairwise(torch::Tensor data, double min_clean, ll v0,
                           ll nv) {
    // pairwise ISC of the voxel window -> r [S (S - 1) / 2, nv], pairs in
    // combinations order (isc_corr_kernels.hip::k_isc_pairwise, k_isc_drop)
    if (nv < 0) nv = data.dim() == 3 ? data.size(1) - v0 : 0;
    check_isc_corr_args(data, v0, nv);
    ll T = data.size(0), V = data.size(1), S = data.size(2);
    TORCH_CHECK(S <= isc_pairwise_max_subjects(), "isc_pairwise needs S <= ",
                isc_pairwise_max_subjects(), " subjects (got ", S, ")");
    auto r = torch::empty({S * (S - 1) / 2, nv}, data.options());
    if (nv == 0) return r;
    TORCH_CHECK(isc_pairwise_blocks(nv, (int)S) <= (ll)INT_MAX,
                "too many blocks for one launch");
    auto flags = torch::empty({nv, S}, data.options().dtype(torch::kUInt8));
    launch_isc_pairwise(data.data_ptr<double>() + v0 * S,
                        r.data_ptr<double>(), flags.data_ptr<uint8_t>(),
                        V * S, T, nv, (int)S, min_clean, cur_stream());
    return r;
}

torch::Tensor searchlight_gram(torch::Tensor x, torch::Tensor mask,
                               torch::Tensor shape, torch::Tensor centres) {
    // per-centre Gram of the searchlight's activity vectors
    // (searchlight_gram.hip::k_sl_gram).  Centre positions are NOT
    // checked here (ops.searchlight_gram checks them on the host).
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 5
                && x.scalar_type() == torch::kFloat32,
                "x must be contiguous fp32 [B,X,Y,Z,E] on the GPU");
    TORCH_CHECK(mask.is_cuda() && mask.is_contiguous() && mask.dim() == 4
                && mask.scalar_type() == torch::kUInt8
                && mask.device() == x.device()
                && mask.sizes() == x.sizes().slice(0, 4),
                "mask must be contiguous uint8 [B,X,Y,Z] on x's GPU");
    TORCH_CHECK(shape.is_cuda() && shape.is_contiguous() && shape.dim() == 3
                && shape.scalar_type() == torch::kUInt8
                && shape.device() == x.device(),
                "shape must be contiguous uint8 [K,K,K] on x's GPU");
    TORCH_CHECK(centres.is_cuda() && centres.is_contiguous()
                && centres.dim() == 1
                && centres.scalar_type() == torch::kInt64
                && centres.device() == x.device(),
                "centres must be contiguous int64 [N] on x's GPU");
    ll K = shape.size(0);
    TORCH_CHECK(shape.size(1) == K && shape.size(2) == K && K % 2 == 1
                && K <= 9, "shape must be cubic with odd K <= 9");
    ll X = x.size(1), Y = x.size(2), Z = x.size(3), E = x.size(4);
    ll N = centres.size(0);
    TORCH_CHECK(E >= 1 && E <= sl_gram_max_e(),
                "searchlight_gram takes 1 <= E <= ", sl_gram_max_e(),
                " (got ", E, ")");
    TORCH_CHECK(X >= K && Y >= K && Z >= K,
                "block smaller than the searchlight shape");
    // offsets inside one block are 32-bit; the block base is 64-bit
    TORCH_CHECK(X * Y * Z <= (ll)INT_MAX, "block too large");
    TORCH_CHECK(N <= (ll)INT_MAX, "too many centres for one launch");
    auto G = torch::empty({N, E, E}, x.options());
    if (N == 0) return G;
    launch_sl_gram(x.data_ptr<float>(), mask.data_ptr<uint8_t>(),
                   shape.data_ptr<uint8_t>(),
                   (const ll*)centres.data_ptr<int64_t>(),
                   G.data_ptr<float>(), N, (int)Y, (int)Z, (int)E, (int)K,
                   cur_stream());
    return G;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("searchlight_gram", &searchlight_gram,
          "per-centre Gram of the searchlight's activity vectors "
          "-> G [N,E,E] fp32",
          pybind11::arg("x"), pybind11::arg("mask"), pybind11::arg("shape"),
          pybind11::arg("centres"));
    m.def("searchlight_gram_max_e", []() { return sl_gram_max_e(); },
          "epoch cap of k_sl_gram");
    m.def("isc_loo", &isc_loo,
          "leave-one-out ISC of data [T,V,S] fp64 -> r [S,nv] fp64",
          pybind11::arg("data"), pybind11::arg("tolerant"),
          pybind11::arg("min_clean") = -1.0, pybind11::arg("v0") = 0,
          pybind11::arg("nv") = -1);
    m.def("isc_pairwise", &isc_pairwise,
          "pairwise ISC of data [T,V,S] fp64 -> r [S(S-1)/2,nv] fp64",
          pybind11::arg("data"), pybind11::arg("min_clean") = -1.0,
          pybind11::arg("v0") = 0, pybind11::arg("nv") = -1);
    m.def("isc_pairwise_max_subjects",
          []() { return isc_pairwise_max_subjects(); },
          "subject cap of k_isc_pairwise");
    m.def("isc_phase_stat", &isc_phase_stat,
          "coef [I,R,K] x table [R,K,V] + nanmedian / Fisher mean over R "
          "-> out [I,V] fp64",
          pybind11::arg("table"), pybind11::arg("coef"),
          pybind11::arg("stat"));
    m.def("isc_phase_max_rows", []() { return isc_phase_max_rows(); },
          "row cap of the median path of k_isc_phase_stat");
    m.def("isc_resample_stat", &isc_resample_stat,
          "per-draw gather + nanmedian / Fisher mean -> out [I,V] fp64",
          pybind11::arg("table"), pybind11::arg("rows"),
          pybind11::arg("lags").none(true), pybind11::arg("signs"),
          pybind11::arg("stat"));
    m.def("isc_resample_max_rows", []() { return isc_resample_max_rows(); },
          "row cap of the median path of k_isc_resample_stat");
    m.def("hmm_forward_backward", &hmm_forward_backward,
          "log-space HMM forward-backward over chain states "
          "-> (log_gamma [B,T,K], ll [B])");
    m.def("hmm_fb_tile", []() { return hmm_fb_tile(); },
          "timesteps per streamed tile of k_hmm_fb");
    m.def("hmm_viterbi", &hmm_viterbi,
          "MAP path over chain states -> (path int32 [B,T], score [B])");
    m.def("hmm_viterbi_tile", []() { return hmm_viterbi_tile(); },
          "timesteps per backtrace tile of k_hmm_viterbi");
    m.def("stencil3d", &stencil3d,
          "direct [K,K,K] valid conv over [B,X,Y,Z] (searchlight ball)");
    m.def("isfc_accum_", &isfc_accum_,
          "acc += atanh(clamp((M + M^T)/2)) fused in one pass");
    m.def("isfc_fused_", &isfc_fused_,
          "acc += atanh(sym(Zs_b Zm_b^T)) per subject, M never "
          "materialized (bf16 MFMA tile pairs)");
    m.def("svm_cv", &svm_cv,
          "batched precomputed-kernel SVC cross-validation",
          py::arg("kernels"), py::arg("y"), py::arg("train_idx"),
          py::arg("test_idx"), py::arg("n_train"), py::arg("n_test"),
          py::arg("C"), py::arg("tol"), py::arg("max_iter"),
          py::arg("max_n") = -1, py::arg("variant") = "auto");
    m.def("svm_cv_trace", &svm_cv_trace,
          "svm_cv through the TRACE kernels: (correct, dec [C,F,E], "
          "n_iter [C,F]); for tests",
          py::arg("kernels"), py::arg("y"), py::arg("train_idx"),
          py::arg("test_idx"), py::arg("n_train"), py::arg("n_test"),
          py::arg("C"), py::arg("tol"), py::arg("max_iter"),
          py::arg("max_n") = -1, py::arg("variant") = "auto");
    m.def("svm_cv_shared_fits",
          [](int64_t E, int64_t max_n) {
              return svm_cv_shared_fits((int)E, (ll)max_n) != 0;
          },
          "true when the shared-tile svm_cv variant covers the shape");
    m.def("fcma_normalize_", &fcma_normalize_,
          "in-place Fisher-z + within-subject z-score [C,E,V]");
    m.def("fcma_correlate", &fcma_correlate,
          "raw chunk correlation [count,E,VB] fp32");
    m.def("fcma_corr_norm_z", &fcma_corr_norm_z,
          "fused corr(+norm) -> Z (bf16/fp8; raw=True defers norm)",
          pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("start"),
          pybind11::arg("count"), pybind11::arg("P"),
          pybind11::arg("padE"),
          pybind11::arg("out") = pybind11::none(),
          pybind11::arg("raw") = false);
    m.def("fcma_gram", &fcma_gram, "per-voxel Gram from fp32 [C,E,V]");
    m.def("debug_fp8_cvt", &debug_fp8_cvt,
          "device to_fp8 conversion probe", pybind11::arg("x"),
          pybind11::arg("sw") = false);
    m.def("fcma_gram_fp8", &fcma_gram_fp8,
          "per-voxel Gram from fp8(e4m3) Z [C,E,V]");
    m.def("fcma_corr_gram_duo", &fcma_corr_gram_duo,
          "one-grid raw-corr(chunk i) + gram(chunk i-1) + partial-sum/"
          "shrink(chunk i-2) co-residency",
          pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("start"),
          pybind11::arg("count"), pybind11::arg("P"),
          pybind11::arg("Zout"),
          pybind11::arg("Zprev") = pybind11::none(),
          pybind11::arg("Gpart") = pybind11::none(),
          pybind11::arg("Gsum_part") = pybind11::none(),
          pybind11::arg("Gsum_out") = pybind11::none(),
          pybind11::arg("shrink") = true);
    m.def("fcma_gram_bf16", &fcma_gram_bf16,
          "per-voxel Gram from bf16 Z [C,E,V]; norm_P>0 applies "
          "Fisher-z + z-score to raw correlations in-tile",
          pybind11::arg("Z"), pybind11::arg("norm_P") = 0);
    m.def("fcma_corr_gram_fused", &fcma_corr_gram_fused,
          "single-kernel corr + normalize + Gram over the cached "
          "[64, V, LP] operands -> [count, 64, 64]",
          py::arg("At_all"), py::arg("B_t"), py::arg("start"),
          py::arg("count"), py::arg("P"), py::arg("nsplit") = 1,
          py::arg("shrink") = true, py::arg("clamp") = "auto",
          py::arg("schedule") = "auto", py::arg("fisher") = "auto");
    m.def("fcma_corr_gram_fused_partials", &fcma_corr_gram_fused_partials,
          "the [nsplit, count, 64, 64] slabs of fcma_corr_gram_fused as "
          "the kernel writes them (unshrunk, not summed)",
          py::arg("At_all"), py::arg("B_t"), py::arg("start"),
          py::arg("count"), py::arg("P"), py::arg("nsplit"),
          py::arg("clamp") = "auto", py::arg("schedule") = "auto",
          py::arg("fisher") = "auto");
    m.def("fcma_corr_gram_fused_table",
          [](int64_t P, int64_t L) {
              return fcma_corr_gram_fused_table((int)P, L) != 0;
          }, "whether the (P, L) instance takes the Fisher z from the LDS "
          "table (clamp \"auto\")");
    m.def("fcma_fisher_table_probe", &fcma_fisher_table_probe,
          "tests only: (table, log-path z, lookup z) for fp32 values r");
    m.def("fcma_fused_image_layout", &fcma_fused_image_layout_py,
          "tests only: (stride, image bytes, table bytes, store offsets, "
          "read offsets) of the fused kernel's z image in LDS",
          py::arg("P"));
    m.def("fcma_corr_gram_fused_ahead",
          [](int64_t P, int64_t L) {
              return fcma_corr_gram_fused_ahead((int)P, L) != 0;
          }, "whether the (P, L) instance has the \"ahead\" schedule");
    m.def("fcma_corr_gram_fused_supported",
          [](int64_t E, int64_t P, int64_t L) {
              return fcma_corr_gram_fused_supported(E, (int)P, L) != 0;
          }, "shape envelope of fcma_corr_gram_fused");
    m.def("fcma_corr_gram_fused_lp",
          [](int64_t L) { return fcma_corr_gram_fused_lp(L); },
          "row length of the fused operands for epoch length L");
    m.def("fcma_corr_gram_fused_cb",
          []() { return fcma_corr_gram_fused_cb(); },
          "selected voxels per fused workgroup");
    m.def("fcma_fused_gram_native", &fcma_fused_gram_native,
          "true when the single-kernel corr+gram path covers (E, P, L)");
    m.def("fcma_fused_gram", &fcma_fused_gram,
          "corr+norm+Gram for a voxel chunk");
    m.def("jacobi_eigh", &jacobi_eigh, "batched KxK symmetric eigensolve");
    m.def("batched_polar", &batched_polar,
          "batched orthogonal Procrustes polar factor");
    m.def("polar_invsqrt", &polar_invsqrt,
          "G^{-1/2} for a stack of SPD KxK Gram matrices");
    m.def("tfa_factor", &tfa_factor, "TFA RBF factor matrix");
    m.def("tfa_recon", &tfa_recon, "TFA residual");
}
