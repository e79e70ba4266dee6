"""GPU tests for the schedule of the single-kernel FCMA path
(k_corr_gram_fused).

``schedule="ahead"`` issues the correlation MFMAs of task t+1 before the
normalize of task t, from column fragments loaded a task earlier still,
so the prefetch of a window's last two tasks reaches into the next
window; ``schedule="phased"`` is the order the kernel was first shipped
with (load one task ahead, MFMA at the head of its own task).  Both run
the same MFMAs on the same operands, so they must agree in every bit,
and so must two launches of the new order.

The shapes are the smallest at which the task pipeline can break: one
window (prologue and run-out with no steady state), two windows of which
the last has a dead 16-column sub-tile (the run-on prefetch meets the
column clamp), three windows, a column split without any window (its
slab must be exactly zero: the prologue must not run), 200 columns cut
1, 2 and 7 ways (the run-on prefetch of a split's last window reads the
next split's columns),
selected counts below and off the 16-voxel tile with a shifted start,
P of 2 and 4, row lengths LP of 16, 32 and 64, padded epoch rows, and a
self-correlation, whose |r| >= 1 diagonal sends tasks of one sweep
through both normalize streams.

Accuracy uses the conventions of test_fcma_fused_feed.py: a CPU oracle
from the same bf16 inputs (r in fp32 rounded to bf16, fp32 normalize, z
rounded to bf16, Gram in fp64), errors per selected voxel (abs = max
|G - ref|, rel = abs / max |ref|) maximised over voxels, and the
streamed path (fcma_corr_norm_z(raw=True) + fcma_gram_bf16(norm_P=P))
as the yardstick: the fused kernel may err at most twice as much, or by
two bf16 rounding events of z in one Gram entry where that is more (the
shapes here are small enough for either path to have none by chance).
Every case is compared with the oracle.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


def _zscored_epochs(g, E, L, V):
    # pad L to the set the streamed kernels take (zero rows are inert)
    Lpad = next(opt for opt in (8, 16, 24, 32, 40) if L <= opt)
    out = torch.zeros((E, Lpad, V), dtype=torch.float32)
    for e in range(E):
        m = torch.randn((L, V), generator=g)
        m = (m - m.mean(0)) / m.std(0, unbiased=False).clamp_min(1e-12)
        out[e, :L] = m / math.sqrt(L)
    return out


def _pad16(B):
    """data2 zero-padded to a multiple of 16 columns, as stack_epochs
    does."""
    E, L, V = B.shape
    Vp = ((V + 15) // 16) * 16
    Bp = torch.zeros((E, L, Vp), dtype=B.dtype)
    Bp[:, :, :V] = B
    return Bp


def _rq(A, B, start, count):
    """bf16-rounded correlations [count, E, V] of the bf16 inputs."""
    corr = torch.einsum('elc,elv->cev',
                        A.float()[:, :, start:start + count], B.float())
    return corr.to(torch.bfloat16).float()


def _ref_normalize(corr, P):
    num = 1.0 + corr
    den = 1.0 - corr
    num = torch.where(num <= 0, torch.full_like(num, 1e-4), num)
    den = torch.where(den <= 0, torch.full_like(den, 1e-4), den)
    z = 0.5 * torch.log(num / den)
    C, E, V = corr.shape
    z = z.view(C, E // P, P, V)
    mean = z.mean(dim=2, keepdim=True)
    var = (z * z).mean(dim=2, keepdim=True) - mean * mean
    inv = torch.where(var > 0, var.rsqrt(), torch.zeros_like(var))
    return ((z - mean) * inv).view(C, E, V)


def _shrink64(G):
    lead = G[:, 0, 0].abs().clamp_min(1.0)
    digits = torch.floor(torch.log10(lead)) + 1
    scale = torch.where(digits > 2, torch.pow(10.0, 2 - digits),
                        torch.ones_like(lead))
    return G * scale[:, None, None]


# (E, L, P, V2, start, count, same, nsplits).  The LP = 64 rows (L = 40)
# have no "ahead" instance: there test_ahead_equals_phased compares the
# phased kernel with itself and only shows that the argument is accepted
# and falls back; their accuracy check is a real one.
CASES = {
    "one_window": (64, 12, 4, 32, 0, 16, False, (1,)),
    "dead_subtile": (64, 12, 4, 48, 0, 16, False, (1, 2)),
    "three_windows": (64, 12, 4, 96, 3, 17, False, (1, 3)),
    "v200_c5": (64, 12, 4, 200, 0, 5, False, (1, 2, 7)),
    "v200_c17": (64, 12, 4, 200, 3, 17, False, (1, 2, 7)),
    "v200_c40": (64, 12, 4, 200, 3, 40, False, (1, 2, 7)),
    "self": (64, 12, 4, 200, 3, 40, True, (1, 2, 7)),
    "p2": (64, 12, 2, 200, 0, 17, False, (1, 2, 7)),
    "p2_lp32": (64, 24, 2, 96, 3, 17, False, (1, 3)),
    "p2_lp64": (64, 40, 2, 48, 0, 5, False, (1, 2)),
    "p4_lp32": (64, 24, 4, 96, 3, 17, False, (1, 3)),
    "p4_lp64": (64, 40, 4, 48, 0, 5, False, (1, 2)),
    "epad": (48, 12, 4, 80, 3, 17, False, (1, 3)),
}


SEED_BASE = 500


@functools.lru_cache(maxsize=None)
def _case(name):
    """bf16 inputs (selected side, data2 padded) and the unshrunk fp64
    oracle Gram of one case; computed once, never modified."""
    E, L, P, V2, start, count, same, _ = CASES[name]
    g = torch.Generator().manual_seed(SEED_BASE + sorted(CASES).index(name))
    B = _zscored_epochs(g, E, L, V2).to(torch.bfloat16)
    A = B if same else _zscored_epochs(g, E, L, V2).to(torch.bfloat16)
    z = _ref_normalize(_rq(A, B, start, count), P)
    z = z.to(torch.bfloat16).double()
    ref = torch.bmm(z, z.transpose(1, 2))
    Bp = _pad16(B)
    Ap = Bp if same else A
    return Ap, Bp, ref


@functools.lru_cache(maxsize=None)
def _operands(ops, name):
    Ap, Bp, _ = _case(name)
    a_t = ops.fcma_fused_operand(Ap.cuda())
    b_t = a_t if Ap is Bp else ops.fcma_fused_operand(Bp.cuda())
    return a_t, b_t


# ---------------------------------------------------------------------------
# 1. the schedule cannot change a bit
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_ahead_equals_phased(ops, name):
    E, L, P, V2, start, count, same, nsplits = CASES[name]
    a_t, b_t = _operands(ops, name)
    assert ops.fcma_corr_gram_fused_supported(E, P, L)
    for nsplit in nsplits:
        for shrink in (True, False):
            for clamp in ("auto", "always"):
                kw = dict(nsplit=nsplit, shrink=shrink, clamp=clamp)
                phased = ops.fcma_corr_gram_fused(
                    a_t, b_t, start, count, P, schedule="phased", **kw)
                ahead = ops.fcma_corr_gram_fused(
                    a_t, b_t, start, count, P, schedule="ahead", **kw)
                again = ops.fcma_corr_gram_fused(
                    a_t, b_t, start, count, P, schedule="ahead", **kw)
                auto = ops.fcma_corr_gram_fused(
                    a_t, b_t, start, count, P, **kw)
                tag = f"nsplit={nsplit} shrink={shrink} clamp={clamp}"
                assert ahead.shape == (count, 64, 64)
                assert bool(torch.isfinite(ahead).all()), tag
                assert torch.equal(ahead, phased), \
                    "schedule changed a bit: " + tag
                assert torch.equal(ahead, again), \
                    "two ahead launches differ: " + tag
                assert torch.equal(auto, phased), tag


def test_short_epochs_take_the_ahead_order(ops):
    # the instances that ship an "ahead" form must not quietly stay
    # phased: LP = 16 (the flagship) and LP = 32, not LP = 64
    for P in (2, 4):
        for L in (8, 12, 16, 17, 24, 32):
            assert ops.fcma_corr_gram_fused_ahead(P, L), (P, L)
        for L in (33, 40, 64):
            assert not ops.fcma_corr_gram_fused_ahead(P, L), (P, L)


def test_schedule_argument_is_checked(ops):
    a_t, b_t = _operands(ops, "one_window")
    with pytest.raises(RuntimeError):
        ops.fcma_corr_gram_fused(a_t, b_t, 0, 16, 4, schedule="eager")


# ---------------------------------------------------------------------------
# 2. a column split without a window
# ---------------------------------------------------------------------------

def _split_inputs(ops, V2, seed):
    g = torch.Generator().manual_seed(seed)
    B = _zscored_epochs(g, 64, 12, V2).to(torch.bfloat16)
    A = _zscored_epochs(g, 64, 12, V2).to(torch.bfloat16)
    return ops.fcma_fused_operand(A.cuda()), ops.fcma_fused_operand(B.cuda())


@pytest.mark.parametrize("schedule", ["ahead", "phased"])
def test_split_without_window(ops, schedule):
    # V2 = 64 is two windows; cut three ways the splits are [0, 1),
    # [1, 2) and the empty [2, 2).  The Gram entry point takes at most
    # one split per window, so this cut is only reachable through the
    # slab view.
    P, start, count = 4, 3, 17
    a_t, b_t = _split_inputs(ops, 64, 64)
    ext = ops.load_extension()
    with pytest.raises(RuntimeError):
        ops.fcma_corr_gram_fused(a_t, b_t, start, count, P, nsplit=3,
                                 schedule=schedule)
    slabs = ext.fcma_corr_gram_fused_partials(a_t, b_t, start, count, P, 3,
                                              schedule=schedule)
    assert slabs.shape == (3, count, 64, 64)
    assert not slabs[2].any(), "the split without a window is not zero"
    # a split's slab is the one-split Gram of its own columns
    for w in range(2):
        alone = ops.fcma_corr_gram_fused(
            a_t, b_t[:, w * 32:(w + 1) * 32].contiguous(), start, count, P,
            shrink=False, schedule=schedule)
        assert alone.any()
        assert torch.equal(slabs[w], alone)
    other = "phased" if schedule == "ahead" else "ahead"
    assert torch.equal(slabs, ext.fcma_corr_gram_fused_partials(
        a_t, b_t, start, count, P, 3, schedule=other))


@pytest.mark.parametrize("schedule", ["ahead", "phased"])
def test_split_without_window_public_entry(ops, schedule):
    # V2 = 160 is five windows; nsplit = 4 gives two windows per split:
    # [0, 2), [2, 4), [4, 5) and a fourth split that starts past the end
    P, start, count = 4, 3, 17
    a_t, b_t = _split_inputs(ops, 160, 160)
    ext = ops.load_extension()
    slabs = ext.fcma_corr_gram_fused_partials(a_t, b_t, start, count, P, 4,
                                              schedule=schedule)
    assert not slabs[3].any(), "the split without a window is not zero"
    assert slabs[0].any() and slabs[1].any() and slabs[2].any()
    G4 = ops.fcma_corr_gram_fused(a_t, b_t, start, count, P, nsplit=4,
                                  shrink=False, schedule=schedule)
    # the reduction adds the slabs in fp32, in split order, from zero
    acc = torch.zeros_like(slabs[0])
    for k in range(4):
        acc = acc + slabs[k]
    assert torch.equal(G4, acc)
    # One split cannot be bitwise the same: there the windows add up
    # inside the MFMA accumulators, here three partial sums are rounded
    # to fp32 and added.  Each of the two orders rounds a running sum of
    # magnitude <= max|G| once per window MFMA (5) or per slab (4) and
    # within an MFMA's 32-term dot product: 64 roundings of 2^-24 bound
    # the gap with room.
    G1 = ops.fcma_corr_gram_fused(a_t, b_t, start, count, P, nsplit=1,
                                  shrink=False, schedule=schedule)
    gap = float((G4 - G1).abs().max())
    bound = 64 * 2.0 ** -24 * float(G1.abs().max())
    print(f"nsplit 4 vs 1 ({schedule}): max gap {gap:.3g}, bound {bound:.3g}")
    assert gap <= bound


# ---------------------------------------------------------------------------
# 3. accuracy still holds
# ---------------------------------------------------------------------------

def _errors(G, ref):
    d = (G - ref).abs().flatten(1).max(dim=1).values
    scale = ref.abs().flatten(1).max(dim=1).values
    return float(d.max()), float((d / scale).max())


def _shrink_scale(G):
    """Per-voxel factor that _shrink64 applies to G."""
    lead = G[:, 0, 0].abs().clamp_min(1.0)
    digits = torch.floor(torch.log10(lead)) + 1
    return torch.where(digits > 2, torch.pow(10.0, 2 - digits),
                       torch.ones_like(lead))


# The fused kernel may err at most twice as much as the streamed path,
# or, where that is the larger, by the floor below.  Both paths err
# against the oracle by discrete events: a z whose fp32 value lies so
# close to a bf16 rounding boundary that the last bits of the normalize
# tip it to the neighbouring bf16 value.  One event moves z by one bf16
# ulp, at most 2^-7 since |z| <= sqrt(P - 1) < 2 for a z-score over P
# values, and a Gram entry by that times a partner z, twice on the
# diagonal: at most 2 * 2^-7 * sqrt(P - 1).  The ratio alone is ill-
# conditioned where a case holds only a few events, because the streamed
# path may by chance have none of any size while the fused path has one
# (and the other way round).  The floor is two such events of the
# largest size and the same sign meeting in one Gram entry, scaled like
# the Gram by the magnitude shrink.  An indexing or hand-over mistake
# moves an entry by whole products z * z' (order 1 per column), far above
# it.
def _flip_floor(P):
    return 2.0 * (2.0 * 2.0 ** -7 * math.sqrt(P - 1))


def _fused_and_streamed_errors(ops, name, schedule=None):
    """(fa, fr, ea, er, floor_a, floor_r) of one case: errors of the
    fused kernel and of the streamed path against the oracle, and the
    absolute / relative floor."""
    E, L, P, V2, start, count, same, _ = CASES[name]
    Ap, Bp, ref0 = _case(name)
    ref = _shrink64(ref0)
    a_t, b_t = _operands(ops, name)
    kw = {} if schedule is None else dict(schedule=schedule)
    G = ops.fcma_corr_gram_fused(a_t, b_t, start, count, P, **kw)
    assert torch.equal(G, G.transpose(1, 2)), "not exactly symmetric"
    if E < 64:      # zero-padded epoch rows stay exactly zero
        assert not G[:, E:, :].any() and not G[:, :, E:].any()
    fa, fr = _errors(G[:, :E, :E].double().cpu(), ref)

    Acu = Ap.cuda().contiguous()
    Bcu = Acu if same else Bp.cuda().contiguous()
    z = torch.zeros((count, 64, Bp.shape[2]), dtype=torch.bfloat16,
                    device="cuda")
    ops.load_extension().fcma_corr_norm_z(Acu, Bcu, start, count, P, 64,
                                          out=z, raw=True)
    Ge = ops.fcma_gram_bf16(z, norm_P=P)[:, :E, :E].double().cpu()
    ea, er = _errors(_shrink64(Ge), ref)

    floor_c = _flip_floor(P) * _shrink_scale(ref0)
    floor_a = float(floor_c.max())
    floor_r = float((floor_c / ref.abs().flatten(1).max(dim=1).values).max())
    return fa, fr, ea, er, floor_a, floor_r


@pytest.mark.parametrize("name", sorted(CASES))
def test_accuracy_vs_streamed_path(ops, name):
    fa, fr, ea, er, floor_a, floor_r = _fused_and_streamed_errors(
        ops, name, schedule="ahead")
    print(f"{name}: fused abs {fa:.4g} rel {fr:.4g} | streamed abs "
          f"{ea:.4g} rel {er:.4g} | ratio abs {fa / max(ea, 1e-30):.3f} "
          f"rel {fr / max(er, 1e-30):.3f} | floor abs {floor_a:.4g} "
          f"rel {floor_r:.4g}")
    assert fa <= max(2.0 * ea, floor_a), (fa, ea, floor_a)
    assert fr <= max(2.0 * er, floor_r), (fr, er, floor_r)
