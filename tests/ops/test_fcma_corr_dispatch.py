"""GPU tests for the (P, L) dispatch of the FCMA correlation launchers.

fcma_kernels.hip maps a runtime (epochs per subject P, epoch length L)
onto one template instantiation per launcher through a single checked
dispatcher.  Every instantiation that a binding can reach is launched
here once, at shapes that cross every tile edge with a tail:

    VA = 144, start = 5, count = 131   (128-voxel dot3s tile, 16/32-voxel
                                        dot2 tiles)
    VB = 272                           (256-column tile + 16 columns)

and all nine epoch lengths 8, 12, ..., 40, generated at that length.

1. Bits against the parent.  tests/ops/data/fcma_corr_dispatch_sha256.json
   holds the SHA-256 of the bytes of every output, recorded from the
   build of the commit before the dispatcher was introduced
   (``python tests/ops/test_fcma_corr_dispatch.py --record``; only
   bindings that both sides have are used).  The kernels were not touched
   by that change, so every digest must be equal.
2. The raw-correlation outputs (fp32 mode 2, bf16 raw, the duo grid's
   bf16 raw) against einsum('elc,elv->cev') of the bf16-rounded inputs in
   fp32, atol = rtol = 2e-2 as in test_correlate_matches_torch (bf16
   rounding of r in [-1, 1] stays below 2^-9).  The normalized outputs
   are held to their oracle by test_corr_norm_z_all_templates.
3. The checked dispatch seen from Python: a P without an instantiation
   raises, every valid (P, L) returns a tensor of the promised shape, and
   an epoch length for which the single-kernel chunk path has no
   instantiation takes the two-kernel composite.
"""

import functools
import hashlib
import json
import os
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(_HERE, "data", "fcma_corr_dispatch_sha256.json")

VA, START, COUNT, VB = 144, 5, 131, 272
START2 = VA - COUNT          # second duo launch: another voxel window
EPAD = 64
LS = (8, 12, 16, 20, 24, 28, 32, 36, 40)
CS_SUM, NSPLIT = 37, 2       # gsum population / Gram column splits


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


# ---------------------------------------------------------------------------
# cases: (kind, P or E, E, L)
#   norm : fcma_corr_norm_z, bf16 out          P in {2,4,8,16,3}, E = 2P
#   raw  : fcma_corr_norm_z(raw=True)          P in {2,4},        E = 2P
#   fp8  : fcma_corr_norm_z into an e4m3 buf   P in {2,4},        E = 2P
#   corr : fcma_correlate (mode 2, fp32)       E in {8,4,6,5} -> P 8,4,2,1
#   duo  : fcma_corr_gram_duo, two launches    P in {2,4}, E in {16,68}
# ---------------------------------------------------------------------------

def _name(kind, P, E, L):
    return f"{kind}_p{P}_e{E}_l{L}"


CASES = {}
for _L in LS:
    for _P in (2, 4, 8, 16, 3):
        CASES[_name("norm", _P, 2 * _P, _L)] = ("norm", _P, 2 * _P, _L)
    for _P in (2, 4):
        CASES[_name("raw", _P, 2 * _P, _L)] = ("raw", _P, 2 * _P, _L)
        CASES[_name("fp8", _P, 2 * _P, _L)] = ("fp8", _P, 2 * _P, _L)
        for _E in (16, 68):
            CASES[_name("duo", _P, _E, _L)] = ("duo", _P, _E, _L)
    for _E, _P in ((8, 8), (4, 4), (6, 2), (5, 1)):
        CASES[_name("corr", _P, _E, _L)] = ("corr", _P, _E, _L)

ORACLE_CASES = sorted(n for n, c in CASES.items()
                      if c[0] in ("raw", "corr", "duo"))


def _zscored(g, E, L, V):
    x = torch.randn((E, L, V), generator=g)
    x = x - x.mean(1, keepdim=True)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """bf16 z-scored epochs A [E, L, VA], B [E, L, VB] of one case, from
    the case's own seed; computed once, never modified."""
    _, _, E, L = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return _zscored(g, E, L, VA), _zscored(g, E, L, VB)


def _epad(E):
    return ((E + 63) // 64) * 64


@functools.lru_cache(maxsize=None)
def _outputs(ops, name):
    """{output name: CPU tensor} of one case, launched once."""
    kind, P, E, L = CASES[name]
    ext = ops.load_extension()
    A, B = (t.cuda() for t in _inputs(name))
    out = {}
    if kind == "norm":
        out["Z"] = ext.fcma_corr_norm_z(A, B, START, COUNT, P, EPAD)
    elif kind in ("raw", "fp8"):
        dt = torch.bfloat16 if kind == "raw" else torch.float8_e4m3fn
        buf = torch.zeros((COUNT, EPAD, VB), dtype=dt, device="cuda")
        out["Z"] = ext.fcma_corr_norm_z(A, B, START, COUNT, P, EPAD,
                                        out=buf, raw=(kind == "raw"))
    elif kind == "corr":
        out["corr"] = ops.fcma_correlate(A, B, START, COUNT)
    else:
        Ep = _epad(E)
        z1 = torch.zeros((COUNT, Ep, VB), dtype=torch.bfloat16,
                         device="cuda")
        # first launch of a sweep: correlation blocks only
        ext.fcma_corr_gram_duo(A, B, START, COUNT, P, z1)
        out["Zout"] = z1
        # second launch: all three block populations
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + 1)
        gsp = (50.0 * torch.randn((NSPLIT, CS_SUM, Ep, Ep),
                                  generator=g)).cuda()
        z2 = torch.zeros_like(z1)
        gp = torch.zeros((NSPLIT, COUNT, Ep, Ep), dtype=torch.float32,
                         device="cuda")
        gso = torch.zeros((CS_SUM, Ep, Ep), dtype=torch.float32,
                          device="cuda")
        ext.fcma_corr_gram_duo(A, B, START2, COUNT, P, z2, Zprev=z1,
                               Gpart=gp, Gsum_part=gsp, Gsum_out=gso,
                               shrink=True)
        out["Zout2"], out["Gpart"], out["Gsum_out"] = z2, gp, gso
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _shapes(name):
    kind, P, E, L = CASES[name]
    if kind in ("norm", "raw", "fp8"):
        return {"Z": (COUNT, EPAD, VB)}
    if kind == "corr":
        return {"corr": (COUNT, E, VB)}
    Ep = _epad(E)
    return {"Zout": (COUNT, Ep, VB), "Zout2": (COUNT, Ep, VB),
            "Gpart": (NSPLIT, COUNT, Ep, Ep), "Gsum_out": (CS_SUM, Ep, Ep)}


def _sha(t):
    t = t.contiguous()
    return hashlib.sha256(
        t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _key(name, what):
    return f"{name}|{what}"


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---------------------------------------------------------------------------
# 1. bits against the parent (and the promised shapes)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_equal_parent(ops, name):
    want = _fixture()
    outs = _outputs(ops, name)
    shapes = _shapes(name)
    assert sorted(outs) == sorted(shapes)
    for what, t in outs.items():
        assert tuple(t.shape) == shapes[what], _key(name, what)
        assert _sha(t) == want[_key(name, what)], \
            "output differs from the parent's: " + _key(name, what)


# ---------------------------------------------------------------------------
# 2. raw correlations against the fp32 einsum of the bf16 inputs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ORACLE_CASES)
def test_raw_correlation_matches_einsum(ops, name):
    kind, P, E, L = CASES[name]
    A, B = _inputs(name)
    outs = _outputs(ops, name)
    got = [(outs["corr" if kind == "corr" else
                 "Z" if kind == "raw" else "Zout"], START)]
    if kind == "duo":
        got.append((outs["Zout2"], START2))
    for t, start in got:
        ref = torch.einsum('elc,elv->cev',
                           A.float()[:, :, start:start + COUNT], B.float())
        r = t.float()
        err = float((r[:, :E] - ref).abs().max())
        print(f"{name} start={start}: max abs err {err:.4g}")
        assert torch.allclose(r[:, :E], ref, atol=2e-2, rtol=2e-2), err
        assert not r[:, E:].any(), "padding rows were written"


# ---------------------------------------------------------------------------
# 3. the checked dispatch seen from Python
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("L", LS)
def test_unsupported_p_raises(ops, L):
    ext = ops.load_extension()
    g = torch.Generator().manual_seed(L)
    A = _zscored(g, 64, L, VA).cuda()
    B = _zscored(g, 64, L, VB).cuda()
    with pytest.raises(RuntimeError):
        ext.fcma_corr_norm_z(A, B, START, COUNT, 64, EPAD)
    torch.cuda.synchronize()


@pytest.mark.parametrize("L", (12, 20))
def test_fused_gram_length_without_instance_takes_composite(ops, L):
    """k_fused_corr_gram exists for L in {8,16,24,32,40} only.  Another
    supported length at E = 64, P = 4 used to pass the launcher's switch
    without a launch and return an uninitialised Gram; it now reports
    itself as not native and runs corr_norm_z + gram_bf16."""
    ext = ops.load_extension()
    assert ext.fcma_fused_gram_native(64, 4, 16)
    assert not ext.fcma_fused_gram_native(64, 4, L)
    g = torch.Generator().manual_seed(100 + L)
    A = _zscored(g, 64, L, VA).cuda()
    B = _zscored(g, 64, L, VB).cuda()
    G = ops.fcma_fused_gram(A, B, START, COUNT, 4)
    Z = ext.fcma_corr_norm_z(A, B, START, COUNT, 4, EPAD)
    assert G.shape == (COUNT, 64, 64)
    assert torch.equal(G, ops.fcma_gram_bf16(Z))


# ---------------------------------------------------------------------------
# recording the fixture (from the build of the commit before the change)
# ---------------------------------------------------------------------------

def _record(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))
    from brainiak_amd import ops as _ops
    assert torch.cuda.is_available() and _ops.load_extension() is not None
    out = {}
    for name in sorted(CASES):
        outs = _outputs(_ops, name)
        shapes = _shapes(name)
        for what, t in outs.items():
            assert tuple(t.shape) == shapes[what], _key(name, what)
            out[_key(name, what)] = _sha(t)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} digests to {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        _record(sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
    else:
        sys.exit("usage: test_fcma_corr_dispatch.py --record [PATH]")
