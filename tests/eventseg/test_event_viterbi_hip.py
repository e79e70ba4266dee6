"""GPU tests for the single-launch HIP Viterbi (``ops.hmm_viterbi`` /
``k_hmm_viterbi``) and its dispatch from ``EventSegment``.

Oracle: the torch recursion of ``EventSegment._viterbi_batch`` run on
the CPU on the same ``lp``.  The requirement is equality, of paths and
of scores, with no tolerance: both sides do the same fp64 additions and
comparisons in the same order and the build uses no fast-math, so a
mismatch is a bug, not rounding.
"""

import numpy as np
import pytest
import torch

from brainiak_amd.eventseg.event import (EventSegment, _ChainGraph,
                                         _viterbi_torch)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from brainiak_amd import ops as _ops
    if _ops.load_extension() is None:
        pytest.fail("HIP extension not built — GPU box must load it")
    return _ops


def _chains(K, chains):
    return np.zeros(K) if chains is None else np.asarray(chains)


def _logprob(B, T, K, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return -torch.randn((B, T, K), generator=g,
                        dtype=torch.float64).abs() * scale


def _oracle(lp_cpu, chains, graph_t=None):
    """The torch recursion on the CPU.  ``graph_t``: sequence length the
    chain graph is built for (default: that of ``lp_cpu``)."""
    B, T, K = lp_cpu.shape
    if graph_t is None:
        es = EventSegment(K, event_chains=_chains(K, chains), device="cpu")
        return es._viterbi_batch(lp_cpu)
    g = _ChainGraph(_chains(K, chains), graph_t, torch.device("cpu"))
    return _viterbi_torch(lp_cpu, g)


def _kernel(ops, lp_cpu, chains, graph_t=None):
    B, T, K = lp_cpu.shape
    g = _ChainGraph(_chains(K, chains), graph_t or T, torch.device("cuda"))
    path, score = ops.hmm_viterbi(
        lp_cpu.cuda(), g.log_start, g.log_end, g.log_self, g.log_adv,
        g.pred, g.succ)
    torch.cuda.synchronize()
    return path.cpu(), score.cpu()


def _check(path, score, ref_path, ref_score):
    assert path.dtype == torch.int32 and score.dtype == torch.float64
    assert path.shape == ref_path.shape and score.shape == ref_score.shape
    assert not torch.isnan(ref_score).any()
    n_diff = int((path.long() != ref_path).sum())
    # -inf - -inf is nan: equal infinities count as no difference
    d_score = float((score - ref_score).nan_to_num().abs().max())
    print(f"path mismatches={n_diff} score max|diff|={d_score:.3e}")
    assert torch.equal(path.long(), ref_path)
    assert torch.equal(score, ref_score)


def _run_case(ops, lp, chains, graph_t=None):
    ref_path, ref_score = _oracle(lp, chains, graph_t)
    path, score = _kernel(ops, lp, chains, graph_t)
    _check(path, score, ref_path, ref_score)
    return path, score


@pytest.mark.parametrize("B,T,K,chains,scale", [
    pytest.param(3, 9, 8, None, 5, id="T=K+1"),
    pytest.param(2, 1, 1, None, 3, id="zero-trip-loops"),
    pytest.param(2, 2, 2, None, 3, id="smallest-recursion"),
    pytest.param(2, 70, 64, None, 3, id="full-wave-K64"),
    pytest.param(2, 70, 63, None, 3, id="edge-lane-K63"),
    pytest.param(2, 70, 33, None, 3, id="edge-lane-K33"),
    pytest.param(2, 40, 6, [1, 0, 1, 0, 0, 1], 3, id="interleaved-chains"),
    pytest.param(130, 50, 8, None, 3, id="many-sequences"),
    pytest.param(2, 1000, 30, None, 50, id="large-magnitude-long-chain"),
])
def test_kernel_equals_cpu_oracle(ops, B, T, K, chains, scale):
    _, score = _run_case(ops, _logprob(B, T, K, scale, 0), chains)
    assert torch.isfinite(score).all()


def test_kernel_no_path_fits(ops):
    """T < K: no path reaches the tail, the score is -inf and the labels
    are whatever the rules give — still equal to the oracle's.  A chain
    graph built for T = 5 itself refuses K = 8 ("Too few timepoints"),
    so both sides get the chain vectors of a 40-step sequence."""
    _, score = _run_case(ops, _logprob(2, 5, 8, 3, 5), None, graph_t=40)
    assert torch.isneginf(score).all()


def test_kernel_flat_observations_tie_rules(ops):
    """lp == 0: every valid path ties mathematically, so the labels hang
    on the tie rules and on the order of the additions."""
    _run_case(ops, torch.zeros((2, 40, 8), dtype=torch.float64), None)


def test_kernel_exact_ties(ops):
    """Ties that are exact in fp64 (see the CPU tests): the self loop
    wins at K=2, T=3; the lowest final state wins among equal chains."""
    path, _ = _run_case(ops, torch.zeros((1, 3, 2), dtype=torch.float64),
                        None)
    assert path[0].tolist() == [0, 1, 1]
    path, _ = _run_case(ops, torch.zeros((2, 4, 3), dtype=torch.float64),
                        [0, 1, 2])
    assert (path == 0).all()


@pytest.mark.parametrize("which", ["forward", "backtrace"])
@pytest.mark.parametrize("t_of_tile", [
    pytest.param(lambda tt: tt - 1, id="TT-1"),
    pytest.param(lambda tt: tt, id="TT"),
    pytest.param(lambda tt: tt + 1, id="TT+1"),
    pytest.param(lambda tt: 2 * tt + 1, id="2TT+1"),
])
def test_kernel_tile_tails(ops, which, t_of_tile):
    """T around both streaming tiles: the lp tile of the forward pass
    and the mask tile of the backtrace."""
    tt = ops.hmm_fb_tile() if which == "forward" else ops.hmm_viterbi_tile()
    assert tt >= 2
    T = t_of_tile(tt)
    _run_case(ops, _logprob(2, T, 8, 3, 1), None)


def test_kernel_rejects_k_above_64(ops):
    lp = _logprob(2, 80, 65, 3, 2)
    g = _ChainGraph(np.zeros(65), 80, torch.device("cuda"))
    with pytest.raises(RuntimeError):
        ops.hmm_viterbi(lp.cuda(), g.log_start, g.log_end, g.log_self,
                        g.log_adv, g.pred, g.succ)


def test_kernel_empty_batch(ops):
    g = _ChainGraph(np.zeros(4), 12, torch.device("cuda"))
    lp = torch.empty((0, 12, 4), dtype=torch.float64, device="cuda")
    path, score = ops.hmm_viterbi(lp, g.log_start, g.log_end, g.log_self,
                                  g.log_adv, g.pred, g.succ)
    assert path.shape == (0, 12) and score.shape == (0,)
    assert path.dtype == torch.int32 and score.dtype == torch.float64


# -- dispatch ---------------------------------------------------------------

@pytest.fixture
def vit_calls(ops, monkeypatch):
    """Counts calls of ops.hmm_viterbi (still running it)."""
    calls = []
    real = ops.hmm_viterbi

    def counted(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ops, "hmm_viterbi", counted)
    return calls


def test_dispatch_uses_kernel_on_gpu(vit_calls):
    lp = _logprob(3, 20, 5, 3, 4)
    ref_path, ref_score = _oracle(lp, None)
    es = EventSegment(5, device="cuda")
    path, score = es._viterbi_batch(lp.cuda())
    assert len(vit_calls) == 1
    assert path.shape == (3, 20) and score.shape == (3,)
    assert path.dtype == torch.int32 and score.dtype == torch.float64
    assert path.is_cuda and score.is_cuda
    _check(path.cpu(), score.cpu(), ref_path, ref_score)
    # compat side effects are set on the kernel path too
    assert es.P.shape == (6, 6)
    assert es.p_start.shape == (6,) and es.p_end.shape == (6,)


def test_dispatch_env_forces_torch(vit_calls, monkeypatch):
    monkeypatch.setenv("BRAINIAK_EVENTSEG_FB", "torch")
    lp = _logprob(3, 20, 5, 3, 4)
    ref_path, ref_score = _oracle(lp, None)
    path, score = EventSegment(5, device="cuda")._viterbi_batch(lp.cuda())
    assert len(vit_calls) == 0
    assert path.is_cuda and score.is_cuda
    assert score.dtype == torch.float64
    assert torch.equal(path.cpu().long(), ref_path)
    assert torch.equal(score.cpu(), ref_score)


def test_dispatch_k65_stays_on_torch(vit_calls):
    lp = _logprob(2, 80, 65, 3, 3)
    ref_path, ref_score = _oracle(lp, None)
    path, score = EventSegment(65, device="cuda")._viterbi_batch(lp.cuda())
    assert len(vit_calls) == 0
    assert path.is_cuda and score.is_cuda
    assert torch.equal(path.cpu().long(), ref_path)
    assert torch.equal(score.cpu(), ref_score)


# -- end to end: kernel path vs torch path, both on the GPU -----------------

def _both_paths(monkeypatch, fn):
    monkeypatch.delenv("BRAINIAK_EVENTSEG_FB", raising=False)
    hip = fn()
    monkeypatch.setenv("BRAINIAK_EVENTSEG_FB", "torch")
    ref = fn()
    monkeypatch.delenv("BRAINIAK_EVENTSEG_FB")
    return hip, ref


def _regions(rng, n=5, K=4, T=60, V=30):
    regions = []
    for _ in range(n):
        bounds = np.sort(rng.choice(np.arange(1, T), K - 1,
                                    replace=False))
        means = rng.randn(K, V)
        seg = np.zeros((T, V))
        prev = 0
        for e, b in enumerate(list(bounds) + [T]):
            seg[prev:b] = means[e]
            prev = b
        regions.append(seg + 0.3 * rng.randn(T, V))
    return regions


def test_decode_regions_kernel_equals_torch_path(vit_calls, seeded_rng,
                                                 monkeypatch):
    regions = _regions(seeded_rng)
    proto = EventSegment(4, n_iter=5, device="cuda")
    models = proto.fit_regions(regions)
    (ev_h, lp_h), (ev_r, lp_r) = _both_paths(
        monkeypatch, lambda: proto.decode_regions(models, regions))
    assert len(vit_calls) == 1            # one launch for the one group
    assert len(ev_h) == len(ev_r) == 5
    for a, b in zip(ev_h, ev_r):
        assert a.dtype == np.int64 and a.shape == (60,)
        assert np.array_equal(a, b)
    assert np.array_equal(lp_h, lp_r)
    assert np.isfinite(lp_h).all()


def test_decode_chains_kernel_equals_torch_path(vit_calls, seeded_rng,
                                                monkeypatch):
    rng = seeded_rng
    T, V = 50, 20
    chains = np.array([0, 0, 1, 1])
    pat = rng.randn(V, 4)
    data = rng.randn(T, V)

    def run():
        es = EventSegment(4, event_chains=chains, device="cuda")
        es.set_event_patterns(pat)
        return es.decode(data, var=1.0)

    (ev_h, lp_h), (ev_r, lp_r) = _both_paths(monkeypatch, run)
    assert len(vit_calls) == 1
    assert ev_h.shape == (T,) and ev_h.dtype == np.int64
    assert np.array_equal(ev_h, ev_r)
    assert lp_h == lp_r
    assert len(np.unique(chains[ev_h])) == 1
