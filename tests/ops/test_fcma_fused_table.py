"""Tests for the Fisher-z table of the single-kernel FCMA path
(k_corr_gram_fused, ``fisher="table"``).

The Fisher z of the fused kernel is a function of a correlation that has
just been rounded to bf16, so of a 16-bit pattern.  With ``fisher="table"``
the unclamped normalize reads its magnitude from a table that every
workgroup builds in LDS with the arithmetic of the log path, and puts the
sign of r onto it:

    index = min(sat_sub(|r| as bf16 bits, 0x3300), 3200)
    entry 0 = +0 (|r| <= 2^-25: 1 + r and 1 - r both round to 1),
    entry i = log2(1 + m) - log2(1 - m) for the magnitude m = 0x3300 + i,
    entry 3200 = NaN (|r| >= 1, infinities, NaNs: the task is normalized
    again with the clamped logs, as on the log path).

None of this may change a bit of any Gram.  The one difference in the z
image that is allowed: a negative r with |r| <= 2^-25 gives -0 where the
log path gives +0, which no Gram entry can see.

1. CPU: the range constants, in fp32 over every bf16 magnitude below 1.
2. Exhaustive: for all 65 536 bf16 patterns the entry the index rule
   selects, with the sign of r, equals the log-path z bit for bit (both
   from the device functions the kernel runs, through a tests-only
   binding); the NaN entry is selected exactly for |r| >= 1, inf, NaN.
3. Whole kernel: ``fisher="table"`` equals ``fisher="log"`` bit for bit
   over P, L, VB (48: a dead sub-tile), nsplit, schedule and shrink.
4. Tiny family: columns of data2 scaled by +-2^-k, k = 14 .. 40, so that
   the correlations straddle 2^-25 with both signs, whole subjects of
   zero z included: table, log and ``clamp="always"`` agree bitwise.
5. Hits: duplicated voxels and self-correlation in the first / last task
   of the first / last window (the cases of test_fcma_fused_trim.py).
6. Grid family: selected voxels are +-1 at one time step and the columns
   carry chosen bf16 values there, so r is that value exactly; every
   table index occurs with both signs and in both halves of a bf16
   pair, |value| >= 1 in sub-tiles of its own, one Gram per 32-column
   window.
"""

import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))

E = 64
COUNT = 16
TAB_LO = 0x3300            # 2^-25
ONE = 0x3F80               # 1.0
TAB_LAST = ONE - TAB_LO    # 3200, the NaN entry
SEED_BASE = 900


def _load(name):
    spec = importlib.util.spec_from_file_location(
        "_fcma_fused_table_" + name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_trim = _load("test_fcma_fused_trim")
_sched = _trim._sched


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


def _bf16_value(pattern):
    """fp32 array of the bf16 bit patterns (uint array)."""
    return (np.asarray(pattern, dtype=np.uint32) << 16).view(np.float32)


# ---------------------------------------------------------------------------
# 1. range constants (CPU)
# ---------------------------------------------------------------------------

def test_range_constants_cpu():
    mags = np.arange(0, ONE, dtype=np.uint32)          # every |r| < 1
    r = _bf16_value(mags)
    one = np.float32(1.0)
    both_one = ((one + r) == one) & ((one - r) == one)
    assert both_one[:TAB_LO + 1].all()
    assert not both_one[TAB_LO + 1]
    assert not both_one[TAB_LO + 1:].any()
    assert float(r[TAB_LO]) == 2.0 ** -25
    assert 0x3F7F - TAB_LO == 3199
    assert TAB_LAST == 3200
    # 1 +- r stays positive below 1: the unclamped logs are finite there
    assert ((one - r) >= np.float32(2.0 ** -8)).all()


# ---------------------------------------------------------------------------
# 2. the table, exhaustively
# ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_table_equals_log_path_for_every_bf16_pattern(ops):
    ext = ops.load_extension()
    pat = np.arange(1 << 16, dtype=np.uint32)
    r = torch.from_numpy(_bf16_value(pat).copy()).cuda()
    tab, zlog, ztab = (t.cpu().numpy().view(np.uint32)
                       for t in ext.fcma_fisher_table_probe(r))
    assert tab.shape == (TAB_LAST + 1,)
    tabf = tab.view(np.float32)
    assert tab[0] == 0                                  # +0
    assert np.isfinite(tabf[:TAB_LAST]).all()
    assert (tabf[1:TAB_LAST] > 0).all()
    assert np.isnan(tabf[TAB_LAST]) and tab[TAB_LAST] >> 31 == 0

    mag = pat & 0x7fff
    sign = (pat >> 15) << 31
    idx = np.minimum(np.maximum(mag.astype(np.int64) - TAB_LO, 0), TAB_LAST)
    # the NaN entry exactly for |r| >= 1, infinities and NaNs
    assert ((idx == TAB_LAST) == (mag >= ONE)).all()
    sel = (tab[idx] & 0x7fffffff) | sign.astype(np.uint32)

    inr = idx < TAB_LAST
    tiny_neg = inr & (sign != 0) & (mag <= TAB_LO)
    same = sel == zlog
    assert same[inr & ~tiny_neg].all(), \
        f"{int((~same[inr & ~tiny_neg]).sum())} patterns differ"
    # negative |r| <= 2^-25: a zero of the other sign, nothing else
    assert (zlog[tiny_neg] == 0).all()
    assert (sel[tiny_neg] == 0x80000000).all()

    # the lookup the kernel runs gives the selected entry, with r in the
    # low half of a bf16 pair and in the high half (the two byte offsets
    # come out of the packed index by different instructions)
    assert ztab.shape == (2, 1 << 16)
    for half in (0, 1):
        assert (ztab[half][inr] == sel[inr]).all(), half
        assert np.isnan(ztab[half].view(np.float32)[~inr]).all(), half


# ---------------------------------------------------------------------------
# launching
# ---------------------------------------------------------------------------

def _variants(ops, a_t, b_t, start, count, P, nsplits, fishers,
              clamps=("auto",)):
    """{(nsplit, shrink, schedule, fisher or clamp): Gram}"""
    out = {}
    for nsplit in nsplits:
        for shrink in (True, False):
            for schedule in ("ahead", "phased"):
                kw = dict(nsplit=nsplit, shrink=shrink, schedule=schedule)
                for fisher in fishers:
                    out[(nsplit, shrink, schedule, fisher)] = \
                        ops.fcma_corr_gram_fused(a_t, b_t, start, count, P,
                                                 fisher=fisher, **kw)
                if "always" in clamps:
                    out[(nsplit, shrink, schedule, "always")] = \
                        ops.fcma_corr_gram_fused(a_t, b_t, start, count, P,
                                                 clamp="always", **kw)
    return out


def _assert_all_equal(grams, base):
    for (nsplit, shrink, schedule, kind), G in grams.items():
        tag = f"nsplit={nsplit} shrink={shrink} {schedule} {kind}"
        assert bool(torch.isfinite(G).all()), "non-finite Gram: " + tag
        assert torch.equal(G, grams[(nsplit, shrink, schedule, base)]), \
            f"{kind} differs from {base}: " + tag


# ---------------------------------------------------------------------------
# 3. table against log, whole kernel
# ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_which_instances_have_a_table(ops):
    # the instances that ship a table must not quietly keep the logs:
    # row lengths 16 (the flagship) and 32; row length 64 keeps them
    for P in (2, 4):
        for L in (8, 12, 16, 17, 24, 32):
            assert ops.fcma_corr_gram_fused_table(P, L), (P, L)
        for L in (33, 40, 64):
            assert not ops.fcma_corr_gram_fused_table(P, L), (P, L)


@pytest.mark.gpu
@pytest.mark.parametrize("VB", (32, 48, 96))
@pytest.mark.parametrize("L", (12, 24, 40))
@pytest.mark.parametrize("P", (2, 4))
def test_table_equals_log(ops, P, L, VB):
    g = torch.Generator().manual_seed(SEED_BASE + 1000 * P + 10 * L + VB)
    B = _sched._zscored_epochs(g, E, L, VB).to(torch.bfloat16)
    A = _sched._zscored_epochs(g, E, L, VB).to(torch.bfloat16)
    a_t = ops.fcma_fused_operand(A.cuda())
    b_t = ops.fcma_fused_operand(B.cuda())
    nsplits = (1, 2) if VB > 32 else (1,)
    if not ops.fcma_corr_gram_fused_table(P, L):
        # no table instance ships for this epoch length: "auto" is the
        # log path and asking for the table is an error, not a fall-back
        with pytest.raises(RuntimeError):
            ops.fcma_corr_gram_fused(a_t, b_t, 0, COUNT, P, fisher="table")
        grams = _variants(ops, a_t, b_t, 0, COUNT, P, nsplits,
                          ("auto", "log"))
        _assert_all_equal(grams, "log")
        return
    grams = _variants(ops, a_t, b_t, 0, COUNT, P, nsplits,
                      ("table", "log", "auto"))
    assert any(bool(G.any()) for G in grams.values())
    _assert_all_equal(grams, "log")


@pytest.mark.gpu
def test_fisher_argument_is_checked(ops):
    g = torch.Generator().manual_seed(SEED_BASE)
    B = _sched._zscored_epochs(g, E, 12, 32).to(torch.bfloat16)
    b_t = ops.fcma_fused_operand(B.cuda())
    with pytest.raises(RuntimeError):
        ops.fcma_corr_gram_fused(b_t, b_t, 0, COUNT, 4, fisher="atanh")
    # the clamp="always" instances keep the logs
    with pytest.raises(RuntimeError):
        ops.fcma_corr_gram_fused(b_t, b_t, 0, COUNT, 4, fisher="table",
                                 clamp="always")


# ---------------------------------------------------------------------------
# 4. tiny family: correlations on both sides of 2^-25, both signs
# ---------------------------------------------------------------------------

_TINY_K = tuple(range(14, 41))
_TINY_VB = 64


@functools.lru_cache(maxsize=None)
def _tiny_case(P):
    g = torch.Generator().manual_seed(SEED_BASE + 50 + P)
    B = _sched._zscored_epochs(g, E, 12, _TINY_VB)
    A = _sched._zscored_epochs(g, E, 12, _TINY_VB)
    # column j: sign (-1)^j, scale 2^-k with k = 14 + j // 2; powers of
    # two, so the scaled column is exact in bf16 and r scales exactly
    for j in range(2 * len(_TINY_K)):
        B[:, :, j] *= (-1.0) ** j * 2.0 ** -_TINY_K[j // 2]
    A = A.to(torch.bfloat16)
    B = B.to(torch.bfloat16)
    return A, B, _sched._rq(A, B, 0, COUNT)


@pytest.mark.parametrize("P", (2, 4))
def test_tiny_inputs_straddle_the_edge(P):
    rq = _tiny_case(P)[2]                               # [count, E, V]
    edge = 2.0 ** -25
    zero = rq.abs() <= edge
    for neg in (False, True):
        side = (rq < 0) if neg else (rq > 0)
        assert (side & zero).any() and (side & ~zero).any()
        # just above the edge as well, within a factor of four
        assert (side & ~zero & (rq.abs() < 4 * edge)).any()
    # whole subjects of zero z, with negative correlations among them
    subj = zero.view(COUNT, E // P, P, -1).all(2)
    assert subj.any()
    neg_in = (rq < 0).view(COUNT, E // P, P, -1).any(2)
    assert (subj & neg_in).any()
    assert not (rq.abs() >= 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("P", (2, 4))
def test_tiny_table_log_always_agree(ops, P):
    A, B, _ = _tiny_case(P)
    a_t = ops.fcma_fused_operand(A.cuda())
    b_t = ops.fcma_fused_operand(B.cuda())
    grams = _variants(ops, a_t, b_t, 0, COUNT, P, (1, 2),
                      ("table", "log"), clamps=("always",))
    assert all(bool(G.any()) for G in grams.values())
    _assert_all_equal(grams, "log")


# ---------------------------------------------------------------------------
# 5. hits: |r| >= 1 in the first / last task of the first / last window
# ---------------------------------------------------------------------------

_HIT_NAMES = tuple(
    f"hit_{kind}_{window}w_{task}t"
    for kind in ("copy", "negated")
    for window in ("first", "last") for task in ("first", "last")
) + ("hit_self_first", "hit_self_last", "hit_p2_l24_scaled_firstw_firstt",
     "hit_p2_l24_scaled_lastw_lastt")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _HIT_NAMES)
def test_hits_table_log_always_agree(ops, name):
    assert name in _trim.HITS
    a_t, b_t = _trim._operands(ops, name)
    start, count, P = _trim._case(name)[3:6]
    grams = _variants(ops, a_t, b_t, start, count, P, (1, 2),
                      ("table", "log"), clamps=("always",))
    _assert_all_equal(grams, "log")
    _assert_all_equal(grams, "always")


# ---------------------------------------------------------------------------
# 6. grid family: every table index, both signs, through the kernel
# ---------------------------------------------------------------------------

# |value| >= 1, finite: 1, the next bf16, 2, 100, the largest bf16
_OUT_OF_RANGE = (0x3F80, 0x3F81, 0x4000, 0x42C8, 0x7F7F)
_GRID_WINDOWS = 5


@functools.lru_cache(maxsize=None)
def _grid_patterns():
    """bf16 patterns [window, E, 32] of the column values.  Windows 0
    and 1 run through the in-range patterns 0x3300 + i, i = 0 .. 3199
    (epoch-major, so the P epochs of a subject differ), windows 2 and 3
    once more in the other column parity; in window 4
    sub-tile 0 holds only |value| >= 1 and sub-tile 1 in-range patterns
    again."""
    pat = np.zeros((_GRID_WINDOWS, E, 32), dtype=np.uint32)
    e, v = np.meshgrid(np.arange(E), np.arange(32), indexing="ij")
    # the parity of the column is the half of its bf16 pair, and the two
    # halves take their table addresses by different instructions:
    # windows 2 and 3 repeat windows 0 and 1 shifted by one column, so
    # that every index goes through both (3200 is even: the wrap keeps
    # the parity)
    for w in (0, 1, 2, 3):
        pat[w] = TAB_LO + ((w % 2) * E * 32 + e * 32 + v + w // 2) % TAB_LAST
    out = np.asarray(_OUT_OF_RANGE, dtype=np.uint32)
    pat[4] = np.where(v < 16, out[(e + v) % len(out)],
                      TAB_LO + (e * 50 + v * 3 + 7) % TAB_LAST)
    return pat


def _grid_operands(L):
    """A: voxel c is (-1)^c at time step 0 and 0 elsewhere, in every
    epoch; B: the chosen values at time step 0.  Then r[c, e, v] is
    +-value exactly."""
    Lpad = 16 if L <= 16 else 24
    A = torch.zeros((E, Lpad, COUNT), dtype=torch.float32)
    A[:, 0, :] = torch.tensor([(-1.0) ** c for c in range(COUNT)])
    vals = torch.from_numpy(_bf16_value(_grid_patterns()).copy())
    Bs = []
    for w in range(_GRID_WINDOWS):
        B = torch.zeros((E, Lpad, 32), dtype=torch.float32)
        B[:, 0, :] = vals[w]
        Bs.append(B.to(torch.bfloat16))
    return A.to(torch.bfloat16), Bs


@pytest.mark.parametrize("P", (2, 4))
def test_grid_inputs_cover_the_table(P):
    pat = _grid_patterns()
    A, Bs = _grid_operands(12)
    seen = {+1: set(), -1: set()}
    halves = {0: set(), 1: set()}
    for w in range(_GRID_WINDOWS):
        # the values survive the bf16 rounding and r is +-value exactly
        back = (Bs[w][:, 0, :].float().numpy().view(np.uint32) >> 16)
        assert (back == pat[w]).all()
        rq = _sched._rq(A, Bs[w], 0, COUNT)
        want = torch.from_numpy(_bf16_value(pat[w]).copy())
        sgn = A[0, 0, :].float()
        assert torch.equal(rq, sgn[:, None, None] * want[None])
        out = pat[w] >= ONE                              # [E, 32]
        # a task is (subject, 16-column sub-tile): never mixed
        t_out = out.reshape(E // P, P, 2, 16)
        any_out = t_out.any(axis=(1, 3))
        all_out = t_out.all(axis=(1, 3))
        assert (any_out == all_out).all()
        for s in (+1, -1):
            seen[s].update((pat[w][~out] - TAB_LO).tolist())
        for half in (0, 1):
            cols = pat[w][:, half::2]
            halves[half].update((cols[cols < ONE] - TAB_LO).tolist())
    assert (pat[4] >= ONE).any() and (pat[4] < ONE).any()
    for s in (+1, -1):
        assert seen[s] == set(range(TAB_LAST))
    # and in both halves of a bf16 pair (even and odd columns)
    for half in (0, 1):
        assert halves[half] == set(range(TAB_LAST)), half
    assert (A[0, 0, :] > 0).any() and (A[0, 0, :] < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("P,L", ((4, 12), (2, 12), (4, 24)))
def test_grid_table_log_always_agree(ops, P, L):
    A, Bs = _grid_operands(L)
    a_t = ops.fcma_fused_operand(A.cuda())
    for w in range(_GRID_WINDOWS):
        b_t = ops.fcma_fused_operand(Bs[w].cuda())
        assert b_t.shape[1] == 32                        # one window
        grams = _variants(ops, a_t, b_t, 0, COUNT, P, (1,),
                          ("table", "log"), clamps=("always",))
        assert all(bool(G.any()) for G in grams.values()), w
        _assert_all_equal(grams, "log")
