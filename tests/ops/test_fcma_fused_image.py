"""Tests for the LDS z image of the single-kernel FCMA path
(k_corr_gram_fused): where the normalize phase stores a window of z and
where the Gram phase reads it.

The image's address arithmetic lives in fcma_fused_image.h.  The kernel
and a host-side hook (``ops.fcma_fused_image_layout``) evaluate the same
functions, so tests 1 and 2 read the kernel's addresses without a launch.

1. Layout algebra.  The 8-byte pieces that all (wave, si, st, p, lane)
   store tile each voxel's 64 rows x 64 B exactly once, inside the image
   and clear of the other voxels and of the second image; the 16 bytes
   the Gram reads for (voxel, row e, chunk q) are the pieces of columns
   8q .. 8q+3 and then 8q+4 .. 8q+7 of that row.
2. Bank model of gfx950's LDS:
     every ds_write: bank (a/4) mod 32, four groups of 16 contiguous
       lanes;
     ds_read_b128: bank (a/4) mod 64, the four 16-lane groups
       {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, {32-35, 44-47, 52-59},
       {36-43, 48-51, 60-63};
     a group costs as many array cycles as the largest number of distinct
     addresses it puts on one bank.
   A store puts at most 2 addresses on a bank within a group (2-way is
   the floor for a 16-byte-aligned voxel stride with all lanes of a group
   on the same 8-byte half), a Gram read at most 1.  The same model on the
   layout this one replaced (stride 4096 + 32 B, chunk ^ (e>>2)&3) gives
   16 and 8 cycles per instruction, 128 x 16 + 64 x 8 = 2560 per window
   and CU: the figure the hardware counters of that build gave
   (SQ_LDS_IDX_ACTIVE less the table gathers), which pins the model.
3. Bits (GPU).  Only addresses changed: every Gram equals, byte for byte,
   the SHA-256 recorded from the build of the commit before the change
   (tests/ops/data/fcma_fused_image_sha256.json; recorded with
   ``python tests/ops/test_fcma_fused_image.py --record`` in a checkout of
   that commit, whose Python interface is the same).  Random z-scored
   operands, so that every voxel of a block, every epoch row, both
   sub-tiles and both image buffers carry different data: C = 16 (a full
   block) and 17 (a one-voxel block behind it), VB = 48 (a dead sub-tile)
   and 64 (two windows), L = 12 / 24 / 40 (the three row lengths),
   P = 2 / 4, both schedules, fisher "table" / "log" and clamp "always",
   one and two column splits, shrink on and off.  One digest per
   (case, nsplit, shrink): at record time all variants had to agree.
   And every case against the fp64 torch reference with the bound of
   test_fcma_fused_stream.py: at most twice the streamed path's error.
"""

import functools
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "data", "fcma_fused_image_sha256.json")

E = 64
NW = 8                      # waves per workgroup
CB = 16                     # voxels per workgroup and image
ROWB = 64                   # bytes per image row: 32 columns of bf16
# static LDS of the table instances before this layout; the SVM CV
# kernel's 16 640 B have to fit beside it on a CU
LDS_CEILING = 144912


def _load(name):
    spec = importlib.util.spec_from_file_location(
        "_fcma_fused_image_" + name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_stream = _load("test_fcma_fused_stream")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


# ---------------------------------------------------------------------------
# the layout as arrays: store[wave, si, st, p, lane], read[voxel, band, lane]
# ---------------------------------------------------------------------------

def _layout(ops, P):
    stride, image, table, store, read = ops.fcma_fused_image_layout(P)
    return (int(stride), int(image), int(table),
            store.numpy().astype(np.int64), read.numpy().astype(np.int64))


def _old_layout(P):
    """The layout this one replaced, from its formulas: voxel stride
    4096 + 32 B, chunk XORed with (e>>2)&3."""
    stride = E * ROWB + 32
    spw = E // P // NW
    lane = np.arange(64)
    l16, q = lane & 15, lane >> 4
    store = np.zeros((NW, spw, 2, P, 64), dtype=np.int64)
    for wv in range(NW):
        swz = ((wv * P) >> 2) & 3
        for si in range(spw):
            for st in range(2):
                for p in range(P):
                    store[wv, si, st, p] = (
                        l16 * stride + wv * P * 64
                        + (((st * 2 + (q >> 1)) ^ swz) << 4) + (q & 1) * 8
                        + (si * NW * P + p) * 64)
    read = np.zeros((CB, 4, 64), dtype=np.int64)
    for c in range(CB):
        for bnd in range(4):
            e = bnd * 16 + l16
            read[c, bnd] = c * stride + e * 64 + ((q ^ ((e >> 2) & 3)) << 4)
    return stride, CB * stride, store, read


# ---------------------------------------------------------------------------
# 1. layout algebra
# ---------------------------------------------------------------------------

def _pieces(P, store):
    """{byte offset: (voxel, row, first column)} of every 8-byte store of
    a window; asserts that no two stores share an offset."""
    out = {}
    spw = E // P // NW
    for wv in range(NW):
        for si in range(spw):
            for st in range(2):
                for p in range(P):
                    for lane in range(64):
                        off = int(store[wv, si, st, p, lane])
                        e = (wv + NW * si) * P + p
                        col = st * 16 + 4 * (lane >> 4)
                        assert off not in out, (wv, si, st, p, lane)
                        out[off] = (lane & 15, e, col)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("P", (2, 4))
def test_layout_algebra(ops, P):
    stride, image, table, store, read = _layout(ops, P)
    assert store.shape == (NW, E // P // NW, 2, P, 64)
    assert read.shape == (CB, 4, 64)
    assert stride % 16 == 0 and (stride // 16) % 2 == 1
    assert image == CB * stride
    assert table % 16 == 0 and table + 2 * image <= LDS_CEILING

    pieces = _pieces(P, store)
    assert len(pieces) == CB * E * 8                # 8 pieces per row
    per_voxel = {c: [] for c in range(CB)}
    for off, (c, e, col) in pieces.items():
        assert off % 8 == 0
        # inside the voxel's own 4096 B, which lie inside the image: no
        # overlap with another voxel or with the second image at `image`
        assert c * stride <= off and off + 8 <= c * stride + E * ROWB
        assert off + 8 <= image
        # and inside the row the reader expects it in
        assert (off - c * stride) // ROWB == e
        per_voxel[c].append(off - c * stride)
    for c in range(CB):
        assert sorted(per_voxel[c]) == list(range(0, E * ROWB, 8)), c

    # the reader: 16 bytes = columns 8q .. 8q+3, then 8q+4 .. 8q+7
    for c in range(CB):
        for bnd in range(4):
            for lane in range(64):
                off = int(read[c, bnd, lane])
                e, q = bnd * 16 + (lane & 15), lane >> 4
                assert off % 16 == 0
                assert pieces[off] == (c, e, 8 * q), (c, bnd, lane)
                assert pieces[off + 8] == (c, e, 8 * q + 4), (c, bnd, lane)


# ---------------------------------------------------------------------------
# 2. bank model
# ---------------------------------------------------------------------------

WRITE_GROUPS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]
WRITE_BANKS = 32
READ128_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]
READ128_BANKS = 64


def _group_ways(addr, groups, nbytes, banks):
    """Per lane group of one wave instruction (addr: 64 byte addresses,
    nbytes per lane): the largest number of distinct dword addresses on
    one bank = the array cycles the group takes."""
    ways = []
    for lanes in groups:
        on_bank = {}
        for lane in lanes:
            for dw in range(int(addr[lane]) // 4,
                            (int(addr[lane]) + nbytes) // 4):
                on_bank.setdefault(dw % banks, set()).add(dw)
        ways.append(max(len(s) for s in on_bank.values()))
    return ways


def _window_cycles(store, read, wave_voxels=2):
    """(worst ways of a store group, worst ways of a read group, cycles of
    every store, cycles of every read) of one window of one workgroup.
    A wave reads its own two voxels."""
    st_cycles, rd_cycles = [], []
    st_worst = rd_worst = 0
    for instr in store.reshape(-1, 64):
        w = _group_ways(instr, WRITE_GROUPS, 8, WRITE_BANKS)
        st_worst = max(st_worst, max(w))
        st_cycles.append(sum(w))
    for instr in read.reshape(-1, 64):
        w = _group_ways(instr, READ128_GROUPS, 16, READ128_BANKS)
        rd_worst = max(rd_worst, max(w))
        rd_cycles.append(sum(w))
    return st_worst, rd_worst, st_cycles, rd_cycles


@pytest.mark.gpu
@pytest.mark.parametrize("P", (2, 4))
def test_bank_model(ops, P):
    stride, image, table, store, read = _layout(ops, P)
    # the table and the first image are 16-byte multiples, so the banks
    # of both images are those of the offsets (image % 128 is checked
    # through the second image's addresses below)
    for base in (table, table + image):
        st_worst, rd_worst, st_cycles, rd_cycles = _window_cycles(
            store + base, read + base)
        assert len(st_cycles) == 128 and len(rd_cycles) == 64
        assert st_worst <= 2, "a store group more than 2-way"
        assert rd_worst <= 1, "a Gram read group with a conflict"
        assert set(st_cycles) == {8} and set(rd_cycles) == {4}
        assert sum(st_cycles) + sum(rd_cycles) == 1280


@pytest.mark.parametrize("P", (2, 4))
def test_bank_model_reproduces_the_replaced_layout(P):
    """The model on the formulas of the layout before this one: 4-way
    stores and 2-way reads, 2560 array cycles per window and CU, what
    that build's counters gave."""
    stride, image, store, read = _old_layout(P)
    for base in (12816, 12816 + image):
        st_worst, rd_worst, st_cycles, rd_cycles = _window_cycles(
            store + base, read + base)
        assert len(st_cycles) == 128 and len(rd_cycles) == 64
        assert st_worst == 4 and rd_worst == 2
        assert set(st_cycles) == {16} and set(rd_cycles) == {8}
        assert sum(st_cycles) + sum(rd_cycles) == 2560
        # of which conflict cycles: 128 x 12 + 64 x 4
        assert sum(st_cycles) - 128 * 4 + sum(rd_cycles) - 64 * 4 == 1792


# ---------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------

SEED_BASE = 1300
CASES = {f"p{P}_l{L}_c{C}_v{VB}": (P, L, C, VB)
         for P in (2, 4) for L in (12, 24, 40)
         for C in (16, 17) for VB in (48, 64)}
NSPLITS = (1, 2)


@functools.lru_cache(maxsize=None)
def _case(name):
    """bf16 inputs and the unshrunk fp64 oracle Gram; computed once, never
    modified."""
    P, L, C, VB = CASES[name]
    g = torch.Generator().manual_seed(
        SEED_BASE + 10000 * P + 100 * L + 10 * (C - 16) + VB // 16)
    B = _stream._zscored_epochs(g, E, L, VB).to(torch.bfloat16)
    A = _stream._zscored_epochs(g, E, L, VB).to(torch.bfloat16)
    corr = torch.einsum('elc,elv->cev', A.float()[:, :, :C], B.float())
    rq = corr.to(torch.bfloat16).float()
    z = _stream._ref_normalize(rq, P).to(torch.bfloat16).double()
    return A, B, torch.bmm(z, z.transpose(1, 2))


def _variants(ops, name):
    """the (schedule, fisher, clamp) combinations the (P, L) instance has"""
    P, L, _, _ = CASES[name]
    schedules = ("ahead", "phased") \
        if ops.fcma_corr_gram_fused_ahead(P, L) else ("phased",)
    kinds = [("log", "auto"), ("log", "always")]
    if ops.fcma_corr_gram_fused_table(P, L):
        kinds.insert(0, ("table", "auto"))
    return [(s, f, c) for s in schedules for f, c in kinds]


@functools.lru_cache(maxsize=None)
def _grams(ops, name):
    """{(nsplit, shrink, schedule, fisher, clamp): Gram}, each launched
    once"""
    P, L, C, VB = CASES[name]
    A, B, _ = _case(name)
    a_t = ops.fcma_fused_operand(A.cuda())
    b_t = ops.fcma_fused_operand(B.cuda())
    out = {}
    for nsplit in NSPLITS:
        for shrink in (True, False):
            for schedule, fisher, clamp in _variants(ops, name):
                out[(nsplit, shrink, schedule, fisher, clamp)] = \
                    ops.fcma_corr_gram_fused(
                        a_t, b_t, 0, C, P, nsplit=nsplit, shrink=shrink,
                        clamp=clamp, schedule=schedule, fisher=fisher)
    return out


def _sha(G):
    return hashlib.sha256(
        G.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _key(name, nsplit, shrink):
    return f"{name}|nsplit={nsplit}|shrink={int(shrink)}"


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_commit_and_covers_the_cases():
    fx = _fixture()
    assert len(fx["recorded_from_commit"]) >= 7
    want = {_key(n, s, k) for n in CASES for s in NSPLITS
            for k in (True, False)}
    assert set(fx["sha256"]) == want


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_equal_parent(ops, name):
    want = _fixture()["sha256"]
    P, L, C, VB = CASES[name]
    seen = set()
    for key, G in _grams(ops, name).items():
        nsplit, shrink = key[:2]
        tag = f"{_key(name, nsplit, shrink)} {key[2:]}"
        assert G.shape == (C, 64, 64), tag
        assert bool(G.any()) and bool(torch.isfinite(G).all()), tag
        assert _sha(G) == want[_key(name, nsplit, shrink)], \
            "Gram differs from the parent's: " + tag
        seen.add(key[2:])
    assert len(seen) == len(_variants(ops, name)) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_accuracy_vs_streamed_path(ops, name):
    """fp64 reference, the bound of test_fcma_fused_stream.py: the fused
    kernel's error is at most twice the streamed path's."""
    P, L, C, VB = CASES[name]
    A, B, ref0 = _case(name)
    z = torch.zeros((C, 64, VB), dtype=torch.bfloat16, device="cuda")
    ops.load_extension().fcma_corr_norm_z(
        A.cuda().contiguous(), B.cuda().contiguous(), 0, C, P, 64, out=z,
        raw=True)
    Ge = ops.fcma_gram_bf16(z, norm_P=P).double().cpu()
    grams = _grams(ops, name)
    for shrink in (True, False):
        ref = _stream._shrink64(ref0) if shrink else ref0
        ea, er = _stream._errors(
            _stream._shrink64(Ge) if shrink else Ge, ref)
        for nsplit in NSPLITS:
            schedule, fisher, clamp = _variants(ops, name)[0]
            G = grams[(nsplit, shrink, schedule, fisher, clamp)]
            assert torch.equal(G, G.transpose(1, 2)), "not symmetric"
            fa, fr = _stream._errors(G.double().cpu(), ref)
            print(f"{_key(name, nsplit, shrink)}: fused abs {fa:.4g} rel "
                  f"{fr:.4g} | streamed abs {ea:.4g} rel {er:.4g}")
            assert fa <= 2.0 * ea, (fa, ea)
            assert fr <= 2.0 * er, (fr, er)


# ---------------------------------------------------------------------------
# recording the fixture (in a checkout of the commit before the change)
# ---------------------------------------------------------------------------

def _record(path, commit):
    sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
    from brainiak_amd import ops as _ops
    assert torch.cuda.is_available() and _ops.load_extension() is not None
    sha = {}
    for name in sorted(CASES):
        grams = _grams(_ops, name)
        for key, G in grams.items():
            nsplit, shrink = key[:2]
            first = grams[(nsplit, shrink) + _variants(_ops, name)[0]]
            assert torch.equal(G, first), (name, key)
            sha[_key(name, nsplit, shrink)] = _sha(first)
    with open(path, "w") as f:
        json.dump({"recorded_from_commit": commit, "sha256": sha}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(sha)} digests to {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--record":
        _record(sys.argv[3] if len(sys.argv) > 3 else FIXTURE, sys.argv[2])
    else:
        sys.exit("usage: test_fcma_fused_image.py --record COMMIT [PATH]")
