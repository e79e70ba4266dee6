"""GPU tests for the single-launch HIP forward-backward
(``ops.hmm_forward_backward`` / ``k_hmm_fb``) and its dispatch from
``EventSegment``.

Oracle: the torch log-space recursion of
``EventSegment._forward_backward_batch`` run on the CPU in fp64 with the
same ``event_chains``.

Tolerance on finite entries: ``16 * T * eps64 * max(1, max|ll|)`` — one
log-add-exp per step, a few ulp each, on values of magnitude up to about
``|ll|``, accumulated linearly in the worst case.
"""

import numpy as np
import pytest
import torch

from brainiak_amd.eventseg.event import EventSegment, _ChainGraph

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)


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


def _oracle(lp_cpu, chains):
    K = lp_cpu.shape[2]
    es = EventSegment(K, event_chains=_chains(K, chains), device="cpu")
    lg, ll = es._forward_backward_batch(lp_cpu)
    return lg.contiguous(), ll


def _kernel(ops, lp_cpu, chains):
    B, T, K = lp_cpu.shape
    g = _ChainGraph(_chains(K, chains), T, torch.device("cuda"))
    lg, ll = ops.hmm_forward_backward(
        lp_cpu.cuda(), g.log_start, g.log_end, g.log_self, g.log_adv,
        g.pred, g.succ)
    torch.cuda.synchronize()
    return lg.cpu(), ll.cpu()


def _check(lg, ll, ref_lg, ref_ll, T):
    assert lg.shape == ref_lg.shape and ll.shape == ref_ll.shape
    assert lg.dtype == torch.float64 and ll.dtype == torch.float64
    assert not torch.isnan(ref_lg).any() and not torch.isnan(ref_ll).any()
    assert not torch.isnan(lg).any()
    assert not torch.isnan(ll).any()
    assert torch.equal(torch.isneginf(lg), torch.isneginf(ref_lg))
    bound = 16 * T * EPS64 * max(1.0, float(ref_ll.abs().max()))
    finite = torch.isfinite(ref_lg)
    err_lg = float((lg[finite] - ref_lg[finite]).abs().max())
    err_ll = float((ll - ref_ll).abs().max())
    err_sum = float((torch.exp(lg).sum(-1) - 1).abs().max())
    print(f"T={T} bound={bound:.3e} err_lg={err_lg:.3e} "
          f"err_ll={err_ll:.3e} err_sum={err_sum:.3e}")
    assert err_lg <= bound
    assert err_ll <= bound
    assert err_sum <= 1e-9


def _run_case(ops, B, T, K, chains, scale, seed=0):
    lp = _logprob(B, T, K, scale, seed)
    ref_lg, ref_ll = _oracle(lp, chains)
    lg, ll = _kernel(ops, lp, chains)
    _check(lg, ll, ref_lg, ref_ll, T)


@pytest.mark.parametrize("B,T,K,chains,scale", [
    pytest.param(3, 9, 8, None, 5, id="structural-neginf-T=K+1"),
    pytest.param(2, 1, 1, None, 3, id="zero-trip-loops"),
    pytest.param(2, 2, 2, None, 3, id="smallest-recursion"),
    pytest.param(2, 70, 64, None, 3, id="full-wave-K64"),
    pytest.param(2, 70, 63, None, 3, id="edge-lane-K63"),
    pytest.param(2, 70, 33, None, 3, id="edge-lane-K33"),
    pytest.param(2, 40, 6, [1, 0, 1, 0, 0, 1], 3, id="interleaved-chains"),
    pytest.param(130, 50, 8, None, 3, id="many-sequences"),
    pytest.param(2, 1000, 30, None, 50, id="large-magnitude-long-chain"),
])
def test_kernel_matches_cpu_oracle(ops, B, T, K, chains, scale):
    _run_case(ops, B, T, K, chains, scale)


@pytest.mark.parametrize("t_of_tile", [
    pytest.param(lambda tt: tt - 1, id="TT-1"),
    pytest.param(lambda tt: tt, id="TT"),
    pytest.param(lambda tt: tt + 1, id="TT+1"),
    pytest.param(lambda tt: 2 * tt + 1, id="2TT+1"),
])
def test_kernel_tile_tails(ops, t_of_tile):
    """T around the kernel's streaming tile: tails and the prefetch past
    the end of the sequence."""
    tt = ops.hmm_fb_tile()
    assert tt >= 2
    _run_case(ops, 2, t_of_tile(tt), 8, None, 3, seed=1)


def test_kernel_rejects_k_above_64(ops):
    lp = _logprob(2, 80, 65, 3, 2)
    g = _ChainGraph(np.zeros(65), 80, torch.device("cuda"))
    with pytest.raises(RuntimeError):
        ops.hmm_forward_backward(lp.cuda(), g.log_start, g.log_end,
                                 g.log_self, g.log_adv, g.pred, g.succ)


def test_kernel_empty_batch(ops):
    g = _ChainGraph(np.zeros(4), 12, torch.device("cuda"))
    lp = torch.empty((0, 12, 4), dtype=torch.float64, device="cuda")
    lg, ll = ops.hmm_forward_backward(lp, g.log_start, g.log_end,
                                      g.log_self, g.log_adv, g.pred,
                                      g.succ)
    assert lg.shape == (0, 12, 4) and ll.shape == (0,)


# -- dispatch ---------------------------------------------------------------

@pytest.fixture
def fb_calls(ops, monkeypatch):
    """Counts calls of ops.hmm_forward_backward (still running it)."""
    calls = []
    real = ops.hmm_forward_backward

    def counted(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(ops, "hmm_forward_backward", counted)
    return calls


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


def test_dispatch_uses_kernel_on_gpu(fb_calls, seeded_rng):
    regions = _regions(seeded_rng, n=3)
    EventSegment(4, n_iter=3, device="cuda").fit_regions(regions)
    assert len(fb_calls) >= 1


def test_dispatch_env_forces_torch(fb_calls, seeded_rng, monkeypatch):
    monkeypatch.setenv("BRAINIAK_EVENTSEG_FB", "torch")
    regions = _regions(seeded_rng, n=3)
    EventSegment(4, n_iter=3, device="cuda").fit_regions(regions)
    assert len(fb_calls) == 0


def test_dispatch_k65_stays_on_torch(fb_calls):
    B, T, K = 2, 80, 65
    lp = _logprob(B, T, K, 3, 3)
    ref_lg, ref_ll = _oracle(lp, None)
    es = EventSegment(K, device="cuda")
    lg, ll = es._forward_backward_batch(lp.cuda())
    assert len(fb_calls) == 0
    assert lg.is_cuda and ll.is_cuda
    _check(lg.cpu().contiguous(), ll.cpu(), ref_lg, ref_ll, T)


def test_dispatch_return_contract(fb_calls):
    lp = _logprob(3, 20, 5, 3, 4).cuda()
    es = EventSegment(5, device="cuda")
    lg, ll = es._forward_backward_batch(lp)
    assert len(fb_calls) == 1
    assert lg.shape == (3, 20, 5) and ll.shape == (3,)
    assert lg.dtype == torch.float64 and ll.dtype == torch.float64
    assert lg.device == lp.device and ll.device == lp.device
    # compat side effects are set on the kernel path too
    assert es.P.shape == (6, 6)
    assert es.p_start.shape == (6,) and es.p_end.shape == (6,)


# -- end to end: kernel path vs torch path, both on the GPU -----------------

def _both_paths(monkeypatch, fn):
    monkeypatch.delenv("BRAINIAK_EVENTSEG_FB", raising=False)
    hip = fn()
    monkeypatch.setenv("BRAINIAK_EVENTSEG_FB", "torch")
    ref = fn()
    monkeypatch.delenv("BRAINIAK_EVENTSEG_FB")
    return hip, ref


def test_fit_regions_kernel_matches_torch_path(ops, seeded_rng,
                                               monkeypatch):
    regions = _regions(seeded_rng)
    hip, ref = _both_paths(
        monkeypatch,
        lambda: EventSegment(4, n_iter=5,
                             device="cuda").fit_regions(regions))
    assert len(hip) == len(ref) == 5
    for mh, mr in zip(hip, ref):
        assert mh.ll_.shape == mr.ll_.shape
        assert np.allclose(mh.segments_[0], mr.segments_[0], atol=1e-6)
        assert np.allclose(mh.event_pat_, mr.event_pat_, atol=1e-6)
        assert np.isclose(mh.ll_[-1, 0], mr.ll_[-1, 0], atol=1e-8)


def test_find_events_chains_kernel_matches_torch_path(ops, seeded_rng,
                                                      monkeypatch):
    rng = seeded_rng
    T, V = 50, 20
    pat = rng.randn(V, 4)
    data = rng.randn(T, V)

    def run():
        es = EventSegment(4, event_chains=np.array([0, 0, 1, 1]),
                          device="cuda")
        es.set_event_patterns(pat)
        return es.find_events(data, var=1.0)

    (seg_h, ll_h), (seg_r, ll_r) = _both_paths(monkeypatch, run)
    assert seg_h.shape == (T, 4)
    assert np.allclose(seg_h, seg_r, atol=1e-6)
    assert np.isclose(ll_h, ll_r, atol=1e-8)


def test_split_merge_fit_kernel_matches_torch_path(ops, seeded_rng,
                                                   monkeypatch):
    rng = seeded_rng
    K, L, V = 5, 8, 20
    patterns = rng.randn(K, V) * 2
    data = np.repeat(patterns, L, axis=0) + 0.5 * rng.randn(K * L, V)

    def run():
        return EventSegment(K, n_iter=5, split_merge=True,
                            split_merge_proposals=2,
                            device="cuda").fit(data.copy())

    hip, ref = _both_paths(monkeypatch, run)
    assert hip.ll_.shape == ref.ll_.shape
    assert np.allclose(hip.segments_[0], ref.segments_[0], atol=1e-6)
    assert np.allclose(hip.event_pat_, ref.event_pat_, atol=1e-6)
    assert np.allclose(hip.ll_[-1], ref.ll_[-1], atol=1e-8)
