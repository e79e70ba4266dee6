"""GPU tests for the trimmed normalize stream of the single-kernel FCMA
path (k_corr_gram_fused).

The kernel no longer searches each task's correlations for |r| >= 1
before it normalizes.  It runs the unclamped Fisher z for every task and
finds a miss afterwards from the variance of the task (NaN exactly when
some 1 +- r was <= 0); the wave then redoes that task with the clamped
form (epoch lengths up to 32) or its tasks of the whole window (above
32).  Columns past the end of data2 are read as zeros
through a range-checked buffer load instead of being clamped to the last
rows and masked, the running sum starts from z[0] instead of 0 + z[0],
and the LDS store addresses are a per-lane base plus an immediate.  None
of this may change a bit of any Gram.

1. Bits against the parent.  tests/ops/data/fcma_fused_trim_sha256.json
   holds the SHA-256 of the Gram bytes of every case, recorded from the
   build of the commit before this change
   (``python tests/ops/test_fcma_fused_trim.py --record``; the Python
   interface is the same on both sides).  One digest per (case, nsplit,
   shrink): at record time the four (schedule, clamp) combinations had
   to agree, and here each of the four is compared with it.
2. A dead sub-tile contributes nothing: VB = 48 must equal the same data
   with 16 hand-zeroed columns appended (VB = 64), although the operand
   row that follows holds columns that correlate strongly.
3. Late clamp detection: ``clamp="auto"`` equals ``clamp="always"`` bit
   for bit with a hit in the first / last task of the first / last
   window, with one and two column splits, and nothing is non-finite.
4. Every case against the CPU oracle with the bound of
   test_fcma_fused_sched.py (at most twice the streamed path's error, or
   two bf16 rounding events of z in one Gram entry); the helpers are
   loaded from that file.

Tasks: wave w of a workgroup takes subjects w, w + 8, ... (index si) and
the two 16-column sub-tiles st of a 32-column window, in the order
(si, st) = (0, 0), (0, 1), (1, 0), ...  A hit in subject s and column v
therefore lands in wave s % 8, task (s // 8, (v % 32) // 16) of window
v // 32.
"""

import functools
import hashlib
import importlib.util
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "data", "fcma_fused_trim_sha256.json")


def _load_sched_helpers():
    spec = importlib.util.spec_from_file_location(
        "_fcma_fused_sched_helpers",
        os.path.join(_HERE, "test_fcma_fused_sched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_sched = _load_sched_helpers()

E = 64
SEED_BASE = 700
SCHEDULES = ("ahead", "phased")
CLAMPS = ("auto", "always")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


# ---------------------------------------------------------------------------
# cases: name -> builder of (A, B, same, start, count, P) with A, B fp32
# [64, Lpad, V] z-scored epochs (before the bf16 rounding)
# ---------------------------------------------------------------------------

def _epochs(seed, L, V):
    g = torch.Generator().manual_seed(SEED_BASE + seed)
    B = _sched._zscored_epochs(g, E, L, V)
    A = _sched._zscored_epochs(g, E, L, V)
    return A, B


def _grid_case(P, L, VB):
    def build():
        A, B = _epochs(1000 * P + 10 * L + VB // 16, L, VB)
        return A, B, False, 0, 16, P
    return build


def _zero_column_case():
    # column 21 of the live second sub-tile is zero in every epoch:
    # r = 0, z = +0, the running sum starts from that z
    A, B = _epochs(1, 12, 48)
    B[:, :, 21] = 0
    return A, B, False, 0, 16, 4


def _next_row_columns(A, B):
    """Make the first 16 columns of B, taken one epoch row later,
    correlate strongly (r about 0.9) and each differently with the
    selected voxels of A: a load of columns VB .. VB + 15 of row e that
    slipped past the range check would read exactly those."""
    Lp = A.shape[1]
    L = int((A[0].abs().sum(1) > 0).sum())
    for j in range(16):
        x = 0.9 * A[:-1, :L, j] + (0.1 + 0.01 * j) * B[1:, :L, j]
        x = x - x.mean(1, keepdim=True)
        x = x / x.norm(dim=1, keepdim=True)
        B[1:, :L, j] = x
    assert B.shape[1] == Lp


def _dead_next_row_case(VB):
    def build():
        A, B = _epochs(2, 12, 48)
        _next_row_columns(A, B)
        if VB == 64:
            B = torch.cat([B, torch.zeros((E, B.shape[1], 16))], dim=2)
            A = torch.cat([A, torch.zeros((E, A.shape[1], 16))], dim=2)
        return A, B, False, 0, 16, 4
    return build


# late clamp detection: P = 4 (two subjects per wave, tasks 0..3),
# VB = 96 (three windows); wave 3
_P_HIT = 4
_VB_HIT = 96
_WAVE = 3
_TRANSFORMS = {
    "copy": lambda x: x,
    "negated": lambda x: -x,
    "scaled": lambda x: 1.02 * x,
}


def _hit_site(window, task, P=_P_HIT):
    si, st = (0, 0) if task == "first" else (E // P // 8 - 1, 1)
    w = 0 if window == "first" else _VB_HIT // 32 - 1
    return _WAVE + 8 * si, w * 32 + st * 16 + 5


def _plant(A, B, kind, s, v, c, P):
    rows = slice(s * P, (s + 1) * P)
    B[rows, :, v] = _TRANSFORMS[kind](A[rows, :, c])


def _hit_case(kind, window, task, P=_P_HIT, L=12):
    def build():
        seed = 20 + 4 * sorted(_TRANSFORMS).index(kind) \
            + 2 * (window == "last") + (task == "last") + 100 * (L // 12 - 1)
        A, B = _epochs(seed, L, _VB_HIT)
        s, v = _hit_site(window, task, P)
        _plant(A, B, kind, s, v, 7, P)
        return A, B, False, 0, 16, P
    return build


def _two_hits_case(L):
    # waves 1 and 6, both in window 1, different sub-tiles and voxels
    def build():
        A, B = _epochs(40 + L, L, _VB_HIT)
        _plant(A, B, "copy", 1, 32 + 3, 2, _P_HIT)
        _plant(A, B, "scaled", 6, 32 + 16 + 9, 11, _P_HIT)
        return A, B, False, 0, 32, _P_HIT
    return build


def _self_case(start, L=12):
    def build():
        _, B = _epochs(50 + start + L, L, _VB_HIT)
        return B, B, True, start, 16, _P_HIT
    return build


GRID = {f"grid_p{P}_l{L}_v{VB}": _grid_case(P, L, VB)
        for P in (2, 4) for L in (12, 24, 40) for VB in (32, 48, 80)}
EDGES = {
    "zero_column": _zero_column_case,
    "dead_next_row_v48": _dead_next_row_case(48),
    "dead_next_row_v64": _dead_next_row_case(64),
}
# name -> (builder, the (subject, column, voxel) sites that must hit)
HITS = {}
for _kind in sorted(_TRANSFORMS):
    for _window in ("first", "last"):
        for _task in ("first", "last"):
            HITS[f"hit_{_kind}_{_window}w_{_task}t"] = (
                _hit_case(_kind, _window, _task),
                [_hit_site(_window, _task) + (7,)])
HITS["hit_two_in_one_window"] = (
    _two_hits_case(12), [(1, 32 + 3, 2), (6, 32 + 16 + 9, 11)])
# the diagonal sits in window 0 / sub-tile 0 and in window 2 / sub-tile 1
HITS["hit_self_first"] = (_self_case(0), None)
HITS["hit_self_last"] = (_self_case(80), None)
# The two-k-step instances (L = 40) redo a whole window where the others
# redo a task, so they get the same hits; and one P = 2 instance (four
# subjects per wave, the last task is (3, 1)) at L = 24.
for _kind in sorted(_TRANSFORMS):
    for _window, _task in (("first", "first"), ("last", "last")):
        HITS[f"hit_l40_{_kind}_{_window}w_{_task}t"] = (
            _hit_case(_kind, _window, _task, L=40),
            [_hit_site(_window, _task) + (7,)])
HITS["hit_l40_two_in_one_window"] = (
    _two_hits_case(40), [(1, 32 + 3, 2), (6, 32 + 16 + 9, 11)])
HITS["hit_l40_self_last"] = (_self_case(80, L=40), None)
for _window, _task in (("first", "first"), ("last", "last")):
    HITS[f"hit_p2_l24_scaled_{_window}w_{_task}t"] = (
        _hit_case("scaled", _window, _task, P=2, L=24),
        [_hit_site(_window, _task, 2) + (7,)])

BUILDERS = dict(GRID)
BUILDERS.update(EDGES)
BUILDERS.update({k: v[0] for k, v in HITS.items()})


@functools.lru_cache(maxsize=None)
def _case(name):
    """bf16 inputs, the bf16-rounded correlations and the unshrunk fp64
    oracle Gram of one case; computed once, never modified."""
    A, B, same, start, count, P = BUILDERS[name]()
    B = B.to(torch.bfloat16)
    A = B if same else A.to(torch.bfloat16)
    rq = _sched._rq(A, B, start, count)
    z = _sched._ref_normalize(rq, P).to(torch.bfloat16).double()
    ref = torch.bmm(z, z.transpose(1, 2))
    return A, B, same, start, count, P, rq, ref


@functools.lru_cache(maxsize=None)
def _operands(ops, name):
    A, B, same = _case(name)[:3]
    b_t = ops.fcma_fused_operand(B.cuda())
    a_t = b_t if same else ops.fcma_fused_operand(A.cuda())
    return a_t, b_t


def _nsplits(name):
    windows = (_case(name)[1].shape[2] + 31) // 32
    return tuple(n for n in (1, 2, 3) if n <= windows)


def _sha(G):
    return hashlib.sha256(
        G.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _key(name, nsplit, shrink):
    return f"{name}|nsplit={nsplit}|shrink={int(shrink)}"


@functools.lru_cache(maxsize=None)
def _grams(ops, name):
    """{(nsplit, shrink, schedule, clamp): Gram} of one case, every
    combination launched once."""
    a_t, b_t = _operands(ops, name)
    start, count, P = _case(name)[3:6]
    out = {}
    for nsplit in _nsplits(name):
        for shrink in (True, False):
            for schedule in SCHEDULES:
                for clamp in CLAMPS:
                    out[(nsplit, shrink, schedule, clamp)] = \
                        ops.fcma_corr_gram_fused(
                            a_t, b_t, start, count, P, nsplit=nsplit,
                            shrink=shrink, clamp=clamp, schedule=schedule)
    return out


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---------------------------------------------------------------------------
# 1. bits against the parent
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_bits_equal_parent(ops, name):
    want = _fixture()
    count = _case(name)[4]
    for (nsplit, shrink, schedule, clamp), G in _grams(ops, name).items():
        tag = f"{_key(name, nsplit, shrink)} {schedule} {clamp}"
        assert G.shape == (count, 64, 64), tag
        assert _sha(G) == want[_key(name, nsplit, shrink)], \
            "Gram differs from the parent's: " + tag


# ---------------------------------------------------------------------------
# 2. a dead sub-tile reads zeros, not the next operand row
# ---------------------------------------------------------------------------

def test_dead_subtile_equals_hand_zeroed_columns(ops):
    # the planted columns do correlate: were they read, r would be ~0.9
    A, B = _case("dead_next_row_v48")[:2]
    leak = torch.einsum('elc,elv->cev', A.float()[:-1, :, :16],
                        B.float()[1:, :, :16])
    assert float(leak.diagonal(dim1=0, dim2=2).abs().min()) > 0.8
    g48 = _grams(ops, "dead_next_row_v48")
    g64 = _grams(ops, "dead_next_row_v64")
    for key, G in g48.items():
        assert G.any()
        assert torch.equal(G, g64[key]), key


# ---------------------------------------------------------------------------
# 3. late clamp detection
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(HITS))
def test_hit_inputs_hit_where_intended(name):
    """The inputs themselves (CPU only): |r| >= 1 on the bf16 grid at
    the planted sites, and nowhere else."""
    sites = HITS[name][1]
    A, B, same, start, count, P, rq, _ = _case(name)
    hit = rq.abs() >= 1.0                       # [count, E, V]
    if sites is None:                           # self-correlation
        diag = torch.zeros_like(hit)
        for c in range(count):
            diag[c, :, start + c] = True
        assert not (hit & ~diag).any()
        # (a diagonal r is sum(bf16(x)^2), which may round to just under
        # 1: not every epoch hits, but every voxel does, in most subjects)
        per_subject = (hit & diag).view(count, E // P, P, -1).any(3).any(2)
        assert per_subject.any(1).all()
        assert float(per_subject.float().mean()) > 0.5
        return
    allowed = torch.zeros_like(hit)
    for s, v, c in sites:
        allowed[c, s * P:(s + 1) * P, v] = True
        assert hit[c, s * P:(s + 1) * P, v].any(), (s, v, c)
    assert not (hit & ~allowed).any()
    if "scaled" in name:
        s, v, c = sites[-1]
        assert float(rq[c, s * P:(s + 1) * P, v].max()) > 1.0
    if "negated" in name:
        s, v, c = sites[0]
        assert float(rq[c, s * P:(s + 1) * P, v].min()) <= -1.0


@pytest.mark.parametrize("name", sorted(HITS))
def test_auto_clamp_equals_always(ops, name):
    grams = _grams(ops, name)
    assert any(n == 2 for n, _, _, _ in grams)
    for (nsplit, shrink, schedule, clamp), G in grams.items():
        tag = f"{_key(name, nsplit, shrink)} {schedule} {clamp}"
        assert bool(torch.isfinite(G).all()), "non-finite Gram: " + tag
        assert torch.equal(G, grams[(nsplit, shrink, schedule, "always")]), \
            "auto and always differ: " + tag


@pytest.mark.parametrize("name", sorted(set(BUILDERS) - set(HITS)))
def test_finite_and_one_result_whatever_the_order(ops, name):
    grams = _grams(ops, name)
    for (nsplit, shrink, schedule, clamp), G in grams.items():
        tag = f"{_key(name, nsplit, shrink)} {schedule} {clamp}"
        assert bool(torch.isfinite(G).all()), "non-finite Gram: " + tag
        assert torch.equal(G, grams[(nsplit, shrink, "phased", "always")]), \
            tag


# ---------------------------------------------------------------------------
# 4. the oracle, with the bound of test_fcma_fused_sched.py
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _streamed(ops, name):
    """Unshrunk Gram of the streamed path (raw correlations + normalizing
    MFMA Gram), on the CPU in fp64."""
    A, B, same, start, count, P = _case(name)[:6]
    Acu = A.cuda().contiguous()
    Bcu = Acu if same else B.cuda().contiguous()
    z = torch.zeros((count, 64, B.shape[2]), dtype=torch.bfloat16,
                    device="cuda")
    ops.load_extension().fcma_corr_norm_z(Acu, Bcu, start, count, P, 64,
                                          out=z, raw=True)
    return ops.fcma_gram_bf16(z, norm_P=P).double().cpu()


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_accuracy_vs_streamed_path(ops, name):
    P, ref0 = _case(name)[5], _case(name)[7]
    Ge = _streamed(ops, name)
    for shrink in (True, False):
        if shrink:
            ref, Gs = _sched._shrink64(ref0), _sched._shrink64(Ge)
            floor_c = _sched._flip_floor(P) * _sched._shrink_scale(ref0)
        else:
            ref, Gs = ref0, Ge
            floor_c = _sched._flip_floor(P) * torch.ones(ref0.shape[0],
                                                         dtype=ref0.dtype)
        ea, er = _sched._errors(Gs, ref)
        floor_a = float(floor_c.max())
        floor_r = float(
            (floor_c / ref.abs().flatten(1).max(dim=1).values).max())
        for nsplit in _nsplits(name):
            G = _grams(ops, name)[(nsplit, shrink, "ahead", "auto")]
            assert torch.equal(G, G.transpose(1, 2)), "not symmetric"
            fa, fr = _sched._errors(G.double().cpu(), ref)
            print(f"{_key(name, nsplit, shrink)}: fused abs {fa:.4g} rel "
                  f"{fr:.4g} | streamed abs {ea:.4g} rel {er:.4g} | floor "
                  f"abs {floor_a:.4g} rel {floor_r:.4g}")
            assert fa <= max(2.0 * ea, floor_a), (fa, ea, floor_a)
            assert fr <= max(2.0 * er, floor_r), (fr, er, floor_r)


# ---------------------------------------------------------------------------
# recording the fixture (from the build of the commit before the change)
# ---------------------------------------------------------------------------

def _record(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
    from brainiak_amd import ops as _ops
    assert torch.cuda.is_available() and _ops.load_extension() is not None
    out = {}
    for name in sorted(BUILDERS):
        grams = _grams(_ops, name)
        for (nsplit, shrink, schedule, clamp), G in grams.items():
            first = grams[(nsplit, shrink, SCHEDULES[0], CLAMPS[0])]
            assert torch.equal(G, first), (name, nsplit, shrink, schedule,
                                           clamp)
            out[_key(name, nsplit, shrink)] = _sha(first)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} digests to {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        _record(sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
    else:
        sys.exit("usage: test_fcma_fused_trim.py --record [PATH]")
