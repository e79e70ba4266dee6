"""GPU tests for the operand feed and the clamp dispatch of the single-
kernel FCMA path (k_corr_gram_fused).

The kernel clamps the Fisher z (max(1 +- r, 1e-4)) only in tasks in
which some lane holds a bf16-rounded correlation with |r| >= 1; every
other task runs an instruction stream without the clamp.  For |r| < 1
on the bf16 grid 1 +- r >= 2^-8, so the clamp is the identity there and
the two streams must agree in every bit.  ``clamp="always"`` forces the
clamped stream for every task and is the yardstick for that claim.

Accuracy uses the conventions of test_fcma_fused_stream.py: a CPU
oracle from the same bf16 inputs (r in fp32 rounded to bf16, fp32
normalize, z rounded to bf16, Gram in fp64), errors taken per selected
voxel (abs = max |G - ref|, rel = abs / max |ref|) and maximised over
voxels, and the streamed path (fcma_corr_norm_z(raw=True) +
fcma_gram_bf16(norm_P=P)) as the yardstick: the fused kernel may err at
most twice as much.
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


# (E, L, P, V2, start, count, same): counts that are no multiple of 16,
# V2 whose last 32-column window has a dead 16-column sub-tile, P of 2
# and 4, row lengths LP of 16, 32 and 64
CASES = {
    "tails": (64, 12, 4, 200, 3, 40, False),
    "self": (64, 12, 4, 200, 3, 40, True),
    "p2": (64, 8, 2, 144, 0, 16, False),
    "lp32": (64, 24, 4, 112, 0, 33, False),
    "lp64": (64, 40, 4, 112, 0, 33, False),
    "epad": (48, 20, 4, 176, 0, 32, False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """bf16 inputs (selected side, data2 padded) and the unshrunk fp64
    oracle Gram of one case; computed once, never modified."""
    E, L, P, V2, start, count, same = CASES[name]
    g = torch.Generator().manual_seed(300 + sorted(CASES).index(name))
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


def _assert_dispatch_exact(ops, a_t, b_t, start, count, P, nsplit, shrink):
    kw = dict(nsplit=nsplit, shrink=shrink)
    always = ops.fcma_corr_gram_fused(a_t, b_t, start, count, P,
                                      clamp="always", **kw)
    auto = ops.fcma_corr_gram_fused(a_t, b_t, start, count, P,
                                    clamp="auto", **kw)
    again = ops.fcma_corr_gram_fused(a_t, b_t, start, count, P, **kw)
    assert auto.shape == (count, 64, 64) and auto.dtype == torch.float32
    assert torch.equal(auto, always), "clamp dispatch changed a bit"
    assert torch.equal(auto, again), "two auto launches differ"
    return auto


# ---------------------------------------------------------------------------
# 1. dispatch cannot change a bit
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_auto_equals_always(ops, name):
    E, L, P, V2, start, count, same = CASES[name]
    a_t, b_t = _operands(ops, name)
    assert ops.fcma_corr_gram_fused_supported(E, P, _case(name)[0].shape[1])
    for nsplit in (1, 3):
        for shrink in (True, False):
            G = _assert_dispatch_exact(ops, a_t, b_t, start, count, P,
                                       nsplit, shrink)
            assert bool(torch.isfinite(G).all())


def test_clamp_argument_is_checked(ops):
    a_t, b_t = _operands(ops, "p2")
    with pytest.raises(RuntimeError):
        ops.fcma_corr_gram_fused(a_t, b_t, 0, 16, 2, clamp="never")


# ---------------------------------------------------------------------------
# 2. the clamped stream is reached off the diagonal
# ---------------------------------------------------------------------------

# selected voxel -> (data2 column, sign).  Column 70 lies in the third
# window, first sub-tile; 45 in the second window, first sub-tile; 52 in
# the second window, second sub-tile.
PLANTED = {5: (70, 1.0), 21: (45, -1.0), 33: (52, 1.0)}


@functools.lru_cache(maxsize=None)
def _planted(nsel, pairs):
    E, L, V2 = 64, 12, 96
    g = torch.Generator().manual_seed(777)
    B = _zscored_epochs(g, E, L, V2).to(torch.bfloat16)
    A = _zscored_epochs(g, E, L, nsel).to(torch.bfloat16).clone()
    for c, (v, sign) in pairs:
        A[:, :, c] = (sign * B[:, :, v].float()).to(torch.bfloat16)
    return A, B


def _check_planted(ops, nsel, pairs, start, count):
    A, B = _planted(nsel, pairs)
    rq = _rq(A, B, start, count)
    hit = rq.abs() >= 1.0                       # [count, E, V2]
    for c, (v, sign) in pairs:
        n = int(hit[c - start, :, v].sum())
        print(f"selected {c} vs column {v}: |rq| >= 1 in {n} of 64 epochs")
        assert n >= 1, "planted pair no longer reaches |r| >= 1"
        assert bool((sign * rq[c - start, :, v] > 0.9).all())
    a_t = ops.fcma_fused_operand(A.cuda())
    b_t = ops.fcma_fused_operand(B.cuda())
    for nsplit in (1, 3):
        G = _assert_dispatch_exact(ops, a_t, b_t, start, count, 4,
                                   nsplit, True)
        assert bool(torch.isfinite(G).all())


def test_clamped_path_off_diagonal(ops):
    _check_planted(ops, 40, tuple(sorted(PLANTED.items())), 0, 40)


def test_clamped_path_single_voxel(ops):
    # one duplicated voxel, count = 1: the 16 voxel lanes of the tile
    # all recompute it, the clamp is needed in one column group only
    _check_planted(ops, 40, ((5, (70, 1.0)),), 5, 1)


def test_clamped_path_single_lane(ops):
    # one duplicated voxel in a full 16-voxel tile: in the tasks of its
    # sub-tile exactly one lane of the wave needs the clamp
    _check_planted(ops, 40, ((21, (45, -1.0)),), 16, 16)


# ---------------------------------------------------------------------------
# 3. accuracy still holds
# ---------------------------------------------------------------------------

def _errors(G, ref):
    d = (G - ref).abs().flatten(1).max(dim=1).values
    scale = ref.abs().flatten(1).max(dim=1).values
    return float(d.max()), float((d / scale).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_accuracy_vs_streamed_path(ops, name):
    E, L, P, V2, start, count, same = CASES[name]
    Ap, Bp, ref = _case(name)
    ref = _shrink64(ref)
    a_t, b_t = _operands(ops, name)
    G = ops.fcma_corr_gram_fused(a_t, b_t, start, count, P)
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
    print(f"{name}: fused abs {fa:.4g} rel {fr:.4g} | streamed abs "
          f"{ea:.4g} rel {er:.4g} | ratio abs {fa / max(ea, 1e-30):.3f} "
          f"rel {fr / max(er, 1e-30):.3f}")
    assert fa <= 2.0 * ea, (fa, ea)
    assert fr <= 2.0 * er, (fr, er)
