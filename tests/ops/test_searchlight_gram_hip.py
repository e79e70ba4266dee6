"""GPU tests of the searchlight Gram kernel (``k_sl_gram``) and of the
CUDA path of ``MVPAVoxelSelector.run``.

The kernel is checked against the torch twin run on the CPU (fp64,
rounded to fp32) with the standard dot-product rounding bound

    |G - G_ref| <= (nv + 2) * 2^-24 * (|X|^T |X|)

where nv is the number of voxels in the searchlight: nv fp32 roundings
of the fmaf chain, plus the reference's own rounding to fp32.
"""

import numpy as np
import pytest
import torch
from sklearn import svm

from brainiak_amd.fcma.mvpa_voxelselector import MVPAVoxelSelector
from brainiak_amd.searchlight import Ball, Cube, Searchlight

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


def _inner_centres(mask, rad, masked_only=True):
    B, X, Y, Z = mask.shape
    inner = torch.zeros_like(mask)
    inner[:, rad:X - rad, rad:Y - rad, rad:Z - rad] = True
    if masked_only:
        inner &= mask
    return inner.reshape(-1).nonzero()[:, 0]


def _case(dims, B, E, rad, shape_cls, seed, density=0.6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, *dims, E), generator=g)
    mask = torch.rand((B, *dims), generator=g) < density
    shape = torch.as_tensor(shape_cls(rad).mask_)
    return x, mask, shape


def _check(ops, x, mask, shape, centres, G):
    """G (from the GPU) against the CPU twin, with the bound above."""
    assert G.is_cuda and G.dtype == torch.float32
    E = x.shape[-1]
    assert G.shape == (centres.shape[0], E, E)
    G = G.cpu()
    ref = ops.searchlight_gram_torch(x, mask, shape, centres).double()
    absref = ops.searchlight_gram_torch(x.abs(), mask, shape,
                                        centres).double()
    nv = ops.searchlight_gram_torch(torch.ones_like(x[..., :1]), mask,
                                    shape, centres).double()
    bound = (nv + 2) * 2.0 ** -24 * absref
    err = (G.double() - ref).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert torch.equal(G, G.transpose(1, 2))
    return nv[:, 0, 0]


def _run_kernel(ops, x, mask, shape, centres):
    return ops.searchlight_gram_kernel(
        x.cuda(), mask.to(torch.uint8).cuda(), shape.to(torch.uint8).cuda(),
        centres.cuda())


@pytest.mark.parametrize("E", [12, 16, 17, 256])
def test_kernel_matches_twin_over_epoch_counts(ops, E):
    # pad columns, one exact tile, one extra tile of pad, the cap
    assert ops.searchlight_gram_max_e() == 256
    x, mask, shape = _case((5, 5, 5), 2, E, 1, Cube, seed=E)
    centres = _inner_centres(mask, 1)
    assert centres.numel() > 8
    G = _run_kernel(ops, x, mask, shape, centres)
    _check(ops, x, mask, shape, centres, G)


@pytest.mark.parametrize("E", [20, 40])
def test_kernel_matches_twin_ball(ops, E):
    x, mask, shape = _case((7, 6, 8), 1, E, 2, Ball, seed=7)
    centres = _inner_centres(mask, 2)
    G = _run_kernel(ops, x, mask, shape, centres)
    nv = _check(ops, x, mask, shape, centres, G)
    assert nv.max() > 16


def test_kernel_full_rad4_cube_many_slabs(ops):
    # one centre, 729 voxels: 22 full slabs and a partial one
    x, mask, shape = _case((9, 9, 9), 1, 16, 4, Cube, seed=9, density=2.0)
    centres = torch.tensor([(4 * 9 + 4) * 9 + 4])
    G = _run_kernel(ops, x, mask, shape, centres)
    nv = _check(ops, x, mask, shape, centres, G)
    assert int(nv[0]) == 729


def test_kernel_lone_voxel_shapes(ops):
    x, mask, shape = _case((5, 5, 5), 2, 16, 1, Cube, seed=11, density=2.0)
    centre = (1, 2, 2, 2)
    lin = ((1 * 5 + 2) * 5 + 2) * 5 + 2
    centres = torch.tensor([lin, lin - 1])
    want = torch.outer(x[centre], x[centre])
    # a ball that holds only its centre
    lone_shape = torch.zeros((3, 3, 3), dtype=torch.bool)
    lone_shape[1, 1, 1] = True
    G = _run_kernel(ops, x, mask, lone_shape, centres)
    nv = _check(ops, x, mask, lone_shape, centres, G)
    assert nv.tolist() == [1, 1]
    assert torch.equal(G[0].cpu(), want)
    # an all-false neighbourhood except the centre; the second centre
    # sees that one voxel only, through its +z neighbour
    lone_mask = torch.zeros_like(mask)
    lone_mask[centre] = True
    G = _run_kernel(ops, x, lone_mask, shape, centres)
    nv = _check(ops, x, lone_mask, shape, centres, G)
    assert nv.tolist() == [1, 1]
    assert torch.equal(G[0].cpu(), want) and torch.equal(G[1].cpu(), want)
    # nothing in the light at all: a zero Gram
    G = _run_kernel(ops, x, torch.zeros_like(mask), shape, centres)
    assert not bool(G.any())


def test_kernel_no_centres(ops):
    x, mask, shape = _case((5, 5, 5), 1, 12, 1, Cube, seed=1)
    G = _run_kernel(ops, x, mask, shape, torch.empty(0, dtype=torch.int64))
    assert G.shape == (0, 12, 12) and G.is_cuda


def test_kernel_many_centres(ops):
    # every inner voxel of 8 blocks in one launch: grid size and centre
    # indexing
    x, mask, shape = _case((12, 12, 12), 8, 16, 1, Cube, seed=13)
    centres = _inner_centres(mask, 1, masked_only=False)
    assert centres.numel() == 8 * 10 ** 3
    G = _run_kernel(ops, x, mask, shape, centres)
    _check(ops, x, mask, shape, centres, G)


def test_kernel_offsets_beyond_2_to_31(ops):
    # x holds more than 2^31 elements; only the last block is filled and
    # read, and is checked against the twin on that block alone
    E, edge = 256, 12
    per_block = edge ** 3 * E
    B = 2 ** 31 // per_block + 2
    assert (B - 1) * per_block > 2 ** 31
    x_last, mask_last, shape = _case((edge,) * 3, 1, E, 1, Cube, seed=17)
    x = torch.empty((B, edge, edge, edge, E), dtype=torch.float32,
                    device="cuda")
    x[-1] = x_last[0].cuda()
    mask = torch.zeros((B, edge, edge, edge), dtype=torch.uint8,
                       device="cuda")
    mask[-1] = mask_last[0].to(torch.uint8).cuda()
    local = _inner_centres(mask_last, 1)[::37]
    centres = local + (B - 1) * edge ** 3
    G = ops.searchlight_gram(x, mask, shape.cuda(), centres.cuda())
    del x
    _check(ops, x_last, mask_last, shape, local, G)


def test_binding_rejects_bad_arguments(ops):
    x, mask, shape = _case((5, 5, 5), 1, 12, 1, Cube, seed=1)
    centres = _inner_centres(mask, 1).cuda()
    x, mask, shape = (x.cuda(), mask.to(torch.uint8).cuda(),
                      shape.to(torch.uint8).cuda())
    kernel = ops.searchlight_gram_kernel
    assert kernel(x, mask, shape, centres).shape[0] == centres.numel()
    with pytest.raises(RuntimeError):
        kernel(x.double(), mask, shape, centres)
    with pytest.raises(RuntimeError):
        kernel(x, mask.bool(), shape, centres)
    with pytest.raises(RuntimeError):
        kernel(x, mask, shape.float(), centres)
    with pytest.raises(RuntimeError):
        kernel(x, mask, shape, centres.int())
    with pytest.raises(RuntimeError):
        kernel(x.transpose(1, 2), mask.transpose(1, 2), shape, centres)
    with pytest.raises(RuntimeError):
        kernel(x, mask, shape[:, :, :2].contiguous(), centres)
    with pytest.raises(RuntimeError):
        kernel(x, mask, torch.ones((2, 2, 2), dtype=torch.uint8,
                                   device="cuda"), centres)
    with pytest.raises(RuntimeError):
        kernel(x.cpu(), mask, shape, centres)
    cap = ops.searchlight_gram_max_e()
    wide = torch.zeros((1, 5, 5, 5, cap + 1), device="cuda")
    with pytest.raises(RuntimeError):
        kernel(wide, mask, shape, centres)


@pytest.fixture
def kernel_calls(ops, monkeypatch):
    """Counts calls of ops.searchlight_gram_kernel (still running it)."""
    monkeypatch.delenv("BRAINIAK_SL_GRAM", raising=False)
    calls = []
    real = ops.searchlight_gram_kernel

    def counted(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ops, "searchlight_gram_kernel", counted)
    return calls


def test_dispatch_uses_kernel_on_gpu(ops, kernel_calls):
    x, mask, shape = _case((5, 5, 5), 2, 12, 1, Cube, seed=2)
    centres = _inner_centres(mask, 1)
    G = ops.searchlight_gram(x.cuda(), mask.cuda(), shape.cuda(),
                             centres.cuda())
    assert len(kernel_calls) == 1
    _check(ops, x, mask, shape, centres, G)
    # CPU tensors never reach it
    ops.searchlight_gram(x, mask, shape, centres)
    assert len(kernel_calls) == 1


def test_dispatch_env_forces_torch(ops, kernel_calls, monkeypatch):
    monkeypatch.setenv("BRAINIAK_SL_GRAM", "torch")
    x, mask, shape = _case((5, 5, 5), 2, 12, 1, Cube, seed=2)
    centres = _inner_centres(mask, 1)
    G = ops.searchlight_gram(x.cuda(), mask.cuda(), shape.cuda(),
                             centres.cuda())
    assert len(kernel_calls) == 0
    _check(ops, x, mask, shape, centres, G)


def test_dispatch_above_cap_goes_to_twin(ops, kernel_calls):
    cap = ops.searchlight_gram_max_e()
    x, mask, shape = _case((4, 4, 4), 1, cap + 1, 1, Cube, seed=3)
    centres = _inner_centres(mask, 1)
    G = ops.searchlight_gram(x.cuda(), mask.cuda(), shape.cuda(),
                             centres.cuda())
    assert len(kernel_calls) == 0
    _check(ops, x, mask, shape, centres, G)


def test_dispatch_checks_centres_on_gpu(ops, kernel_calls):
    x, mask, shape = _case((5, 5, 5), 2, 12, 1, Cube, seed=2)
    with pytest.raises(ValueError):
        ops.searchlight_gram(x.cuda(), mask.cuda(), shape.cuda(),
                             torch.tensor([31, 4], device="cuda"))
    assert len(kernel_calls) == 0


def test_run_on_cuda_matches_host_path(ops, kernel_calls):
    dims, E = (7, 7, 7), 16
    rng = np.random.RandomState(0)
    mask = rng.rand(*dims) < 0.7
    labels = np.array([e % 2 for e in range(E)])
    data = rng.randn(*dims, E).astype(np.float32)
    data[3, 3, 3, :] += 3.0 * labels
    data[3, 3, 2, :] += 3.0 * labels

    def selector():
        sl = Searchlight(sl_rad=1, max_blk_edge=4, shape=Cube, pool_size=1)
        return MVPAVoxelSelector(data, mask, labels, num_folds=4, sl=sl)

    clf = svm.SVC(kernel='linear', shrinking=False, C=1)
    vol_host, _ = selector().run(clf)
    vol_cuda, ranked = selector().run(clf, device="cuda")
    assert len(kernel_calls) >= 1
    none_host = np.array([v is None for v in vol_host.ravel()])
    none_cuda = np.array([v is None for v in vol_cuda.ravel()])
    assert np.array_equal(none_cuda, none_host)
    host = vol_host.ravel()[~none_host].astype(float)
    cuda = vol_cuda.ravel()[~none_cuda].astype(float)
    diff = cuda - host
    print("max |acc_cuda - acc_host| = %.4f, mean difference = %.4f"
          % (np.abs(diff).max(), diff.mean()))
    assert np.abs(diff).max() <= 0.15
    assert abs(diff.mean()) < 0.05
    assert len(ranked) == int(mask.sum())
    coords = np.array(np.where(mask)).T
    best_vid, best_acc = ranked[0]
    assert best_acc > 0.8
    assert np.abs(coords[best_vid] - np.array([3, 3, 3])).max() <= 2
